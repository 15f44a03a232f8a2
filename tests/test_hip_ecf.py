"""ECF (ecf) on the GPU: the product class against the G20 fixture of the real reference, both forms of the fused affiliation kernels
against float64 under the three-way criterion of tests/test_hip_acf.py

    err(GPU, truth) <= KAPPA * max(err(torch-CPU fp32, 16 threads), err(torch-CPU fp32, 1 thread)) + REL_FLOOR * ||truth||

(err = 2-norm of the difference per tensor; KAPPA and REL_FLOOR are that file's values; the measured ratios are printed), the tie rule, the
all-ones mask, the range errors, the deterministic mode, full-catalogue evaluation on the fp32 route and one end-to-end fit."""
import json
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import ecf_ref
from golden_util import GOLDEN, I, close, load, state_dict
import scorer_truth_util as T
from test_ecf_cpu import KEYS, OTHER_KEYS, _dataset
from test_hip_acf import KAPPA, REL_FLOOR, Report, _with_threads

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = dict(rtol=1e-4, atol=1e-5)                                 # tests/test_hip_acf.py
CASES = json.load(open(os.path.join(GOLDEN, 'g20_ecf.json')))['cases']
NEAR_TIE, NEAR_TIE_CAP = 1e-5, 0.03                              # cosine form: float64 boundary gap below which a row is left out; its cap


def S():
    import sibrar_amd
    return sibrar_amd


def _lib():
    return import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')


def _loss(kind, n_items=I, neg=3):
    cls = {'bce': S().RecBinaryCrossEntropy, 'bpr': S().RecBayesianPersonalizedRankingLoss}[kind]
    return cls(n_items=n_items, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=neg)


# ---- 1. golden parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_g20_ecf_on_hip_kernels(case):
    """The product class == the real reference on every G20 case: train-mode logits, every loss-dictionary entry, BCE and BPR loss,
    every gradient of rec_loss + reg_loss under each loss, evaluation scores through get_*_representations + combine, the pre_tune /
    post_tune outputs of both sides."""
    z = load('g20_ecf')
    name = case['name']
    m = S().ALGORITHMS['ecf'].build_from_conf(case['conf'], _dataset(z))
    sd = state_dict(z, f'{name}/sd/')
    assert list(m.state_dict().keys()) == KEYS and case['keys'] == ['interaction_matrix'] + KEYS
    m.load_state_dict(sd)
    m.to(DEV).train()
    u, i, labels = (torch.from_numpy(z[k]).to(DEV) for k in ('u', 'i', 'labels'))
    for kind in ('bce', 'bpr'):
        m.zero_grad()
        logits = m(u, i)
        close(logits.detach().cpu(), z[f'{name}/logits'], what='logits', **TOL)
        loss = _loss(kind).compute_loss(logits, labels)
        close(loss.detach().cpu(), z[f'{name}/loss_{kind}'], what=f'{kind} loss', **TOL)
        other = m.get_and_reset_other_loss()
        assert list(other) == case['other_keys'] == OTHER_KEYS
        for k, v in other.items():
            assert v.is_cuda, f'{k} left the device'
            close(v.detach().cpu(), z[f'{name}/other_{kind}/{k}'], what=f'{kind} {k}', **TOL)
        (loss + other['reg_loss']).backward()
        for k, p in m.named_parameters():
            close(p.grad.cpu(), z[f'{name}/grad_{kind}/{k}'], what=f'{kind} grad {k}', rtol=1e-4, atol=1e-6, norm_rtol=1e-4)
    m.eval()
    fresh = S().ALGORITHMS['ecf'].build_from_conf(case['conf'], _dataset(z)).to(DEV)
    with pytest.raises(RuntimeError, match='get_item_representations'):
        fresh.get_user_representations(u)                                   # needs a preceding item call
    with torch.no_grad():
        ir = m.get_item_representations(torch.arange(I, device=DEV))
        assert len(ir) == 2
        scores = m.combine_user_item_representations(m.get_user_representations(u), ir)
        close(scores.cpu(), z[f'{name}/scores_all'], what='all-pairs scores', **TOL)
        i_pre, u_pre = m.get_item_representations_pre_tune(i), m.get_user_representations_pre_tune(u)
        i_post, u_post = m.get_item_representations_post_tune(i_pre), m.get_user_representations_post_tune(u_pre)
        assert i_post is i_pre and u_post is u_pre
        for n in (0, 1):
            close(i_post[n].cpu(), z[f'{name}/item_pre_tune/{n}'], what=f'item pre_tune [{n}]', **TOL)
            close(u_post[n].cpu(), z[f'{name}/user_pre_tune/{n}'], what=f'user pre_tune [{n}]', **TOL)


# ---- 2. the kernels against float64 -------------------------------------------------------------------------------------------------
SHAPES = [(200, 8, 6, 2), (1000, 100, 64, 20), (515, 512, 256, 20), (257, 33, 65, 64), (2048, 128, 256, 128), (130, 2, 2, 1), (130, 33, 130, 20)]
TEMP = 2.0


def _cos_cpu(W, Cl, G, Gt, top, dtype, mask=None):
    """(t, x, dW, dCl) of sum(x * G) + sum(t * Gt) by torch autograd; ``mask``: use this mask instead of the dtype's own top-k"""
    w, c = W.to(dtype).clone().requires_grad_(True), Cl.to(dtype).clone().requires_grad_(True)
    t = ecf_ref.cosine_sim(w, c)
    m = ecf_ref.top_mask(t, top) if mask is None else mask.to(dtype)
    p = torch.softmax(t / TEMP, dim=-1)
    x = torch.sigmoid(t) * (p + (m - p).detach())
    ((x * G.to(dtype)).sum() + (t * Gt.to(dtype)).sum()).backward()
    return t.detach(), x.detach(), w.grad, c.grad


def _cos_gpu(W, Cl, G, Gt, top):
    w, c = W.to(DEV).requires_grad_(True), Cl.to(DEV).requires_grad_(True)
    t, x = S().ops.ClusterAffilFn.apply(w, c, None, top, TEMP)
    ((x * G.to(DEV)).sum() + (t * Gt.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    return t.detach().cpu(), x.detach().cpu(), w.grad.cpu(), c.grad.cpu()


@pytest.mark.parametrize('R,D,C,top', SHAPES)
def test_cluster_affil_cosine_form_against_float64(R, D, C, top):
    """t, x, dW and dCl of ops.ClusterAffilFn (cosine form, with an upstream gradient into t) against torch autograd in float64. Rows
    whose float64 gap at the mask boundary is below 1e-5 are left out (their upstream gradients are zeroed, so they reach neither dW nor
    dCl, and their rows of t and x are not compared); their share is capped at 3 % and asserted first."""
    gen = torch.Generator().manual_seed(R + D + C + top)
    W, Cl = torch.randn(R, D, generator=gen), torch.randn(C, D, generator=gen)
    G, Gt = torch.randn(R, C, generator=gen) / R, torch.randn(R, C, generator=gen) / R
    t64 = ecf_ref.cosine_sim(W.double(), Cl.double())
    keep = ecf_ref.gap(t64, top) >= NEAR_TIE
    share = 1.0 - float(keep.double().mean())
    print(f'\nnear-tie rows left out at {(R, D, C, top)}: {share:.4f}')
    assert share <= NEAR_TIE_CAP
    G, Gt = G * keep[:, None], Gt * keep[:, None]
    truth = _cos_cpu(W, Cl, G, Gt, top, torch.float64)
    cpu16 = _with_threads(16, lambda: _cos_cpu(W, Cl, G, Gt, top, torch.float32))
    cpu1 = _with_threads(1, lambda: _cos_cpu(W, Cl, G, Gt, top, torch.float32))
    gpu = _cos_gpu(W, Cl, G, Gt, top)
    rep = Report(f'cluster_affil cosine form R={R} D={D} C={C} top={top}')
    for n, what in enumerate(('t', 'x', 'dW', 'dCl')):
        sel = (lambda a: a[keep]) if n < 2 else (lambda a: a)
        rep.kappa(what, sel(gpu[n]), sel(cpu16[n]), sel(cpu1[n]), sel(truth[n]))
    rep.finish()
    # exactly 0 off the mask, exactly `top` entries on it, and the evaluation form gives the same bits
    assert bool(((gpu[1] != 0).sum(dim=1) == top).all())
    t_e, x_e = S().ops.cluster_affil(W.to(DEV), Cl.to(DEV), None, top, TEMP)
    assert torch.equal(t_e.cpu(), gpu[0]) and torch.equal(x_e.cpu(), gpu[1])


def _logit_cpu(t, G, top, dtype):
    tt = t.to(dtype).clone().requires_grad_(True)
    x = ecf_ref.affiliation(tt, top, TEMP)
    (x * G.to(dtype)).sum().backward()
    return x.detach(), tt.grad


@pytest.mark.parametrize('R,D,C,top', SHAPES)
def test_cluster_affil_logit_form_against_float64(R, D, C, top):
    """x and dt of the logit form on N(0, 2) logits: both sides read the same fp32 values, so the mask is exact (asserted)"""
    gen = torch.Generator().manual_seed(R + C + top)
    t = torch.randn(R, C, generator=gen) * 2.0
    G = torch.randn(R, C, generator=gen) / R
    truth = _logit_cpu(t, G, top, torch.float64)
    cpu16 = _with_threads(16, lambda: _logit_cpu(t, G, top, torch.float32))
    cpu1 = _with_threads(1, lambda: _logit_cpu(t, G, top, torch.float32))
    tg = t.to(DEV).requires_grad_(True)
    x = S().ops.ClusterAffilFn.apply(None, None, tg, top, TEMP)
    (x * G.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    gpu = (x.detach().cpu(), tg.grad.cpu())
    assert torch.equal(gpu[0] != 0, ecf_ref.top_mask(t, top) != 0), 'the mask is exact'
    rep = Report(f'cluster_affil logit form R={R} C={C} top={top}')
    for n, what in enumerate(('x', 'dt')):
        rep.kappa(what, gpu[n], cpu16[n], cpu1[n], truth[n])
    rep.finish()
    assert torch.equal(S().ops.cluster_affil(None, None, t.to(DEV), top, TEMP).cpu(), gpu[0])


# ---- 3. the tie rule, the all-ones mask ------------------------------------------------------------------------------------------------
def test_tie_rule_lowest_index_at_one_dimension():
    """D = 1: every cosine is exactly +-1, so the mask must hold the lowest-index +1 clusters (then the lowest-index -1 clusters)"""
    gen = torch.Generator().manual_seed(3)
    for C, top in ((70, 9), (256, 100), (5, 5), (130, 129)):
        W = torch.randn(150, 1, generator=gen)
        Cl = torch.randn(C, 1, generator=gen)
        t, x = S().ops.cluster_affil(W.to(DEV), Cl.to(DEV), None, top, TEMP)
        t, x = t.cpu(), x.cpu()
        assert bool((t.abs() == 1).all()) and torch.equal(t, torch.sign(W) * torch.sign(Cl).T)
        assert torch.equal(x != 0, ecf_ref.top_mask(t, top) != 0), (C, top)
    # the logit form, rows of equal values and of two values
    t = torch.zeros(70, 200)
    t[1::2, ::3] = 1.
    t[5] = -0.0
    t[5, ::2] = 0.0
    x = S().ops.cluster_affil(None, None, t.to(DEV), 90, TEMP).cpu()
    assert torch.equal(x != 0, ecf_ref.top_mask(t, 90) != 0)


def test_all_ones_mask():
    """top = C: mh = p + (1 - p) everywhere, x = sigmoid(t) to an ulp, nothing is zero"""
    gen = torch.Generator().manual_seed(4)
    t = torch.randn(100, 37, generator=gen)
    x = S().ops.cluster_affil(None, None, t.to(DEV), 37, TEMP).cpu()
    assert bool((x != 0).all())
    close(x, torch.sigmoid(t.double()), what='x at the all-ones mask', rtol=1e-6, atol=0, norm_rtol=0)


# ---- 4. range errors, R = 0 ---------------------------------------------------------------------------------------------------------------
def test_cluster_affil_range_errors_and_no_rows():
    ops = S().ops
    z8, z4 = torch.zeros(4, 8, device=DEV), torch.zeros(4, 4, device=DEV)
    for args, what in (((torch.zeros(3, 513, device=DEV), torch.zeros(4, 513, device=DEV), None, 2, 2.), 'embedding_dim'),
                       ((z8, torch.zeros(1, 8, device=DEV), None, 1, 2.), 'n_clusters'), ((None, None, z4, 5, 2.), 'top'),
                       ((None, None, z4, 0, 2.), 'top'), ((None, None, z4, 2, 0.), 'temp')):
        with pytest.raises(ValueError, match=what):
            ops.cluster_affil(*args)
    L = _lib()
    x = torch.zeros(4, 8, device=DEV)
    for C, top, temp in ((257, 2, 2.), (1, 1, 2.), (8, 9, 2.), (8, 0, 2.), (8, 2, 0.)):      # the entry point itself refuses
        with pytest.raises(S().SibrarHipError, match='n_clusters'):
            L.call('sbr_cluster_affil_fwd', None, 0, None, x.data_ptr(), 4, 0, C, top, temp, None, x.data_ptr(), None, None, None, 0, L.stream())
    with pytest.raises(S().SibrarHipError, match='D'):
        L.call('sbr_cluster_affil_fwd', x.data_ptr(), 8, x.data_ptr(), None, 4, 513, 4, 2, 2., None, x.data_ptr(), None, None, None, 0, L.stream())
    with pytest.raises(S().SibrarHipError, match='n_clusters'):
        L.call('sbr_cluster_affil_bwd', x.data_ptr(), None, None, 0, None, x.data_ptr(), 4, 0, 257, 2., x.data_ptr(), x.data_ptr(), None, 0,
               None, x.data_ptr(), None, 0, L.stream())
    dc = torch.ones(4, 8, device=DEV)      # R = 0 at the entry point: an empty table has no storage, so W is NULL; dCl is zeroed
    L.call('sbr_cluster_affil_bwd', None, None, None, 8, x.data_ptr(), None, 0, 8, 4, 2., None, None, None, 8, dc.data_ptr(), None, None, 0,
           L.stream())
    L.call('sbr_cluster_affil_fwd', None, 8, x.data_ptr(), None, 0, 8, 4, 2, 2., None, None, None, None, None, 0, L.stream())
    assert not bool(dc.any())
    L.CALL_LOG = []
    try:
        w = torch.zeros(0, 8, device=DEV, requires_grad=True)
        c = torch.randn(4, 8, device=DEV, requires_grad=True)
        t, xx = ops.ClusterAffilFn.apply(w, c, None, 2, 2.)
        assert tuple(t.shape) == (0, 4) and tuple(xx.shape) == (0, 4)
        (t.sum() + xx.sum()).backward()
        names = [n for n, _ in L.CALL_LOG]
    finally:
        L.CALL_LOG = None
    assert 'sbr_cluster_affil_fwd' not in names and 'sbr_cluster_affil_bwd' not in names
    assert tuple(w.grad.shape) == (0, 8) and tuple(c.grad.shape) == (4, 8) and not bool(c.grad.any())


# ---- 5. deterministic mode ----------------------------------------------------------------------------------------------------------------
def _ecf_world(n_users, n_items, nnz, seed, n_tags=30, **ds_kw):
    Sm = S()
    ds = Sm.SyntheticDataset(n_users, n_items, nnz, seed=seed, **ds_kw)
    rng = np.random.default_rng(seed)
    item_idx = np.repeat(np.arange(n_items), 2)
    tag_idx = np.concatenate([np.arange(n_items) % n_tags, rng.integers(0, n_tags, size=n_items)]).reshape(2, -1).T.reshape(-1)
    ds.tag_matrix = Sm.ecf_tag_matrix(n_items, item_idx, tag_idx, n_tags)
    return ds


def _train_20(seed):
    Sm = S()
    Sm.reproducible(seed)
    ds = _ecf_world(1000, 1500, 30000, 1, n_negative_samples=3)
    net = Sm.ALGORITHMS['ecf'].build_from_conf(dict(embedding_dim=32, n_clusters=16, top_n=5, top_m=5), ds)
    conf = {'learn': {'lr': 1e-3, 'wd': 1e-4, 'optimizer': 'adamw'}, 'run_settings': {'device': DEV}}
    tr = Sm.Trainer(net, None, None, _loss('bpr', 1500), conf)
    net.train()
    it = iter(Sm.NegativeSamplingDataLoader(ds, batch_size=256, shuffle=True))
    for _ in range(20):
        tr.train_step(*next(it))
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def test_ecf_deterministic_training_is_bit_identical():
    ops = S().ops
    prev = ops.is_deterministic()
    try:
        ops.nondeterministic_launches(reset=True)
        a = _train_20(123)
        b = _train_20(123)
        assert ops.nondeterministic_launches() == 0
        assert ops.is_deterministic()
        assert list(a) == KEYS
        for k in a:
            assert torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)), k
            assert bool(torch.isfinite(a[k]).all())
    finally:
        ops.set_deterministic(prev)


def test_ecf_deterministic_mode_refuses_a_cluster_count_that_is_no_multiple_of_four():
    Sm = S()
    ops = Sm.ops
    prev = ops.set_deterministic(True)
    try:
        ds = _ecf_world(200, 150, 3000, 2, n_negative_samples=3)
        net = Sm.ECF.build_from_conf(dict(embedding_dim=8, n_clusters=6, top_n=2, top_m=2), ds).to(DEV).train()
        u, i, _ = next(iter(Sm.NegativeSamplingDataLoader(ds, batch_size=32, shuffle=False)))
        out = net(u.to(DEV), i.to(DEV))
        with pytest.raises(Sm.SibrarHipError, match='no deterministic form'):
            (out.sum() + net.get_and_reset_other_loss()['reg_loss']).backward()
    finally:
        ops.set_deterministic(prev)


# ---- 6. evaluation ----------------------------------------------------------------------------------------------------------------------
def test_ecf_evaluation_lists_against_the_restatement():
    """400 users x 600 items on the fp32 route (both sides are tuples: ECF scores through its own combine) against the float64
    restatement's ranking with the near-tie acceptance of tests/scorer_truth_util.py. Tolerance of one score, relative to
    sum_c |a_c x_c|: a cosine carries (D + 8) 2^-24, a user logit sums L of them (L = the longest interaction row), sigmoid and the
    softmax mask are 1-Lipschitz in relative terms here, and the dot product adds the fp32 route's 72: ((L + 1) (D + 8) + L + 80) 2^-24.
    Precondition (asserted): no float64 mask boundary closer than 1e-4, so no mask can differ."""
    Sm = S()
    D, C, top = 16, 8, 3
    ds = _ecf_world(400, 600, 8000, 4, n_negative_samples=3, holdout_per_user=1)
    torch.manual_seed(23)                                        # picked on the CPU: the precondition below holds
    net = Sm.ECF.build_from_conf(dict(embedding_dim=D, n_clusters=C, top_n=top, top_m=top), ds).to(DEV).eval()
    view = ds.eval_view()
    sd = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    inter = torch.from_numpy(ds.user_sampling_matrix_train.toarray().astype(np.float64))
    conf = dict(n_clusters=C, top_n=top, top_m=top)
    users = torch.arange(400)
    with torch.no_grad():
        x_tildes, xs = ecf_ref.items(sd, conf)
        a_tilde, a = ecf_ref.users(sd, conf, inter, users, x_tildes)
    assert float(ecf_ref.gap(x_tildes, top).min()) >= 1e-4 and float(ecf_ref.gap(a_tilde, top).min()) >= 1e-4
    scores = (a @ xs.T).to(DEV)
    excluded = torch.from_numpy(view.exclude_data.toarray() != 0).to(DEV)
    masked = scores.masked_fill(excluded, -float('inf'))
    ev = Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=(1, 10, 20)), dataset=view)
    got = []
    loader = type('L', (), {'dataset': view, 'batch_size': 128})()
    L = _lib()
    L.CALL_LOG = []
    try:
        Sm.evaluation._score_split(net, loader, ev, DEV, 'fp32', None, False, 32, lambda s, u_, v, ix: got.append((v, ix)))
        names = {n for n, _ in L.CALL_LOG}
    finally:
        L.CALL_LOG = None
    assert 'sbr_cluster_affil_fwd' in names and not any(n.startswith('sbr_score_topk_f') for n in names), names
    lists = (torch.cat([g[0] for g in got]), torch.cat([g[1] for g in got]))
    longest = int(inter.sum(dim=1).max())
    rel = ((longest + 1) * (D + 8) + longest + 80) * 2.0 ** -24
    T.check_against_truth(lists, users.to(DEV), masked, rel * (a.abs() @ xs.abs().T).to(DEV), 20, what='ecf fp32')
    res = Sm.evaluate_recommender_algorithm(net, loader, Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=(10,)), dataset=view), DEV)
    assert np.isfinite(res['ndcg@10']) and 0.0 <= res['ndcg@10'] <= 1.0


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------------------
def test_ecf_fit_end_to_end(tmp_path):
    Sm = S()
    torch.manual_seed(0)
    np.random.seed(0)
    ds = _ecf_world(500, 300, 15000, 2, n_negative_samples=4, holdout_per_user=1)
    net = Sm.ALGORITHMS['ecf'].build_from_conf(dict(embedding_dim=24, n_clusters=12, top_n=4, top_m=4), ds)
    loader = Sm.NegativeSamplingDataLoader(ds, batch_size=256, shuffle=True)
    val = type('L', (), {'dataset': ds.eval_view(), 'batch_size': 256})()
    conf = {'learn': {'lr': 1e-2, 'wd': 0., 'optimizer': 'adam', 'n_epochs': 2}, 'run_settings': {'device': DEV},
            'eval': Sm.evaluation._Cfg(top_k=(10,)), 'results_path': str(tmp_path)}
    tr = Sm.Trainer(net, loader, val, _loss('bce', 300, 4), conf)
    first = tr.train()
    best = tr.fit()
    assert np.isfinite(best['ndcg@10']) and 0.0 <= best['ndcg@10'] <= 1.0
    last = tr.train()
    assert list(last) == ['train/loss', 'train/rec_loss', 'train/reg_loss', 'train/cf_loss', 'train/ind_loss', 'train/ts_loss']
    assert all(np.isfinite(v) for v in last.values()) and all(np.isfinite(v) for v in first.values())
    assert last['train/loss'] < first['train/loss'], (first, last)
