"""DeepMatrixFactorization on the GPU: the product class against the G17 fixture of the real reference, the cosine scorer kernels and the
whole model against float64 under the three-way criterion of tests/test_hip_c1.py

    err(GPU, truth) <= KAPPA * max(err(torch-CPU fp32, 16 threads), err(torch-CPU fp32, 1 thread)) + floor

(err = 2-norm of the difference per tensor; KAPPA and the floors fixed before measuring; the measured ratios are printed), full-catalogue
evaluation on all three scorer routes against the float64 cosine, the deterministic mode, and one end-to-end fit."""
import json
import os

import numpy as np
import pytest
import torch

import deepmf_ref
import evalk_ref
from golden_util import GOLDEN, I, close, host_dataset, load, state_dict, world
from oracle import losses_ref
import scorer_truth_util as T

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = dict(rtol=1e-4, atol=1e-5)                                 # tests/test_hip_golden.py
CASES = json.load(open(os.path.join(GOLDEN, 'g17_deepmf.json')))['cases']
KAPPA = 3.0
REL_FLOOR = 1e-7                                                 # floor = REL_FLOOR * ||truth|| (tests/test_hip_c1.py)
THREADS = torch.get_num_threads()


def S():
    import sibrar_amd
    return sibrar_amd


def _loss(kind, n_items=I, neg=3):
    cls = {'bce': S().RecBinaryCrossEntropy, 'bpr': S().RecBayesianPersonalizedRankingLoss}[kind]
    return cls(n_items=n_items, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=neg)


def _err(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm())


class Report:
    def __init__(self, title):
        self.title, self.lines, self.bad, self.worst = title, [], [], {}

    def kappa(self, what, gpu, cpu16, cpu1, truth, group=None):
        assert bool(torch.isfinite(gpu).all()), f'{what}: not finite'
        e_gpu, e16, e1 = _err(gpu, truth), _err(cpu16, truth), _err(cpu1, truth)
        floor = REL_FLOOR * float(truth.double().norm())
        cpu = max(e16, e1)
        ok = e_gpu <= KAPPA * cpu + floor
        ratio = e_gpu / cpu if cpu > 0 else (0.0 if e_gpu == 0 else float('inf'))
        line = f'{what:<60} gpu {e_gpu:.3e}  cpu16 {e16:.3e}  cpu1 {e1:.3e}  ratio {ratio:6.2f}  floor {floor:.2e}{"" if ok else "  FAIL"}'
        self.lines.append(line)
        self.worst[group or what] = max(self.worst.get(group or what, 0.0), ratio)
        if not ok:
            self.bad.append(line)

    def finish(self):
        print(f'\n== {self.title}')
        print('\n'.join(self.lines))
        print('largest ratio per tensor:', {k: round(v, 2) for k, v in self.worst.items()})
        assert not self.bad, f'{self.title}: {len(self.bad)} comparison(s) fail:\n' + '\n'.join(self.bad)


def _with_threads(n, fn):
    torch.set_num_threads(n)
    try:
        return fn()
    finally:
        torch.set_num_threads(THREADS)


# ---- 1. golden parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_g17_deepmf_on_hip_kernels(case):
    """The product class == the real reference on every G17 case: train-mode logits, the floored fraction, BCE and BPR loss, every
    gradient under each loss, evaluation scores through get_*_representations + combine."""
    z = load('g17_deepmf')
    name = case['name']
    m = S().ALGORITHMS['dmf'].build_from_conf(case['kwargs'], host_dataset(world(z)))
    sd = state_dict(z, f'{name}/sd/')
    assert list(m.state_dict().keys()) == list(sd.keys())
    m.load_state_dict(sd)
    m.to(DEV).train()
    u, i, labels = (torch.from_numpy(z[k]).to(DEV) for k in ('u', 'i', 'labels'))
    for kind in ('bce', 'bpr'):
        m.zero_grad()
        logits = m(u, i)
        close(logits.detach().cpu(), z[f'{name}/logits'], what='logits', **TOL)
        assert float((logits.detach() == m.mu).double().mean()) == case['floored_fraction']
        loss = _loss(kind).compute_loss(logits, labels)
        close(loss.detach().cpu(), z[f'{name}/loss_{kind}'], what=f'{kind} loss', **TOL)
        loss.backward()
        for k, p in m.named_parameters():
            close(p.grad.cpu(), z[f'{name}/grad_{kind}/{k}'], what=f'{kind} grad {k}', rtol=1e-4, atol=1e-6, norm_rtol=1e-4)
    m.eval()
    with torch.no_grad():
        ir = m.get_item_representations(torch.arange(I, device=DEV))
        scores = m.combine_user_item_representations(m.get_user_representations(u), ir)
    close(scores.cpu(), z[f'{name}/scores_all'], what='all-pairs scores', **TOL)


# ---- 2. the scorer kernels against float64 ------------------------------------------------------------------------------------------
def _cos_cpu(u, i, g, mu, dtype):
    u, i = u.detach().to(dtype).clone().requires_grad_(True), i.detach().to(dtype).clone().requires_grad_(True)
    out = deepmf_ref.combine(u, i, mu)
    out.backward(g.to(dtype))
    return out.detach(), u.grad, i.grad


@pytest.mark.parametrize('D,mu', [(8, 1e-6), (37, 1e-6), (64, 1e-6), (128, 1e-6), (37, -1.0), (64, -1.0)])
def test_score_cos_kernels_against_float64(D, mu):
    """sbr_score_cos_fwd / _bwd at B = 4096, N = 1 + 3 against nn.CosineSimilarity + floor in float64; one row of u and some item rows
    are exactly zero and one row of u and two item rows have norms of 1e-9 .. 3e-10, below eps (mu = -1: the floor is idle, so these rows
    reach the backward pass and take the gradient torch's autograd gives for the clamp, norm term included)."""
    B, N = 4096, 4
    g_ = torch.Generator().manual_seed(D)
    u, i, g = torch.randn(B, D, generator=g_), torch.randn(B, N, D, generator=g_), torch.randn(B, N, generator=g_)
    u[7] = 0
    i[3, 1] = 0
    i[7, 2] = 0
    i[100, 0] = 0
    u[9] *= 1e-9 / float(u[9].norm())                               # 0 < |row| < eps: the clamp is active AND the norm has a gradient
    i[11, 2] *= 3e-10 / float(i[11, 2].norm())
    i[9, 1] *= 2e-9 / float(i[9, 1].norm())
    zero = torch.zeros(B, N, dtype=torch.bool)                      # entries that touch a clamped norm
    zero[7, :] = zero[9, :] = zero[3, 1] = zero[100, 0] = zero[11, 2] = True
    truth = _cos_cpu(u, i, g, mu, torch.float64)
    cpu16 = _with_threads(16, lambda: _cos_cpu(u, i, g, mu, torch.float32))
    cpu1 = _with_threads(1, lambda: _cos_cpu(u, i, g, mu, torch.float32))
    ud, idv = u.detach().to(DEV).requires_grad_(True), i.detach().to(DEV).requires_grad_(True)
    out = S().ops.ScoreCosFn.apply(ud, idv, mu)
    out.backward(g.to(DEV))
    gpu = (out.detach().cpu(), ud.grad.cpu(), idv.grad.cpu())
    assert all(bool(torch.isfinite(t).all()) for t in gpu)
    rep = Report(f'score_cos D={D} mu={mu}')
    # rows that touch a clamped norm carry gradients of order 1 / eps = 1e8: they are compared on their own so that they do not drown the rest
    urow = zero.any(1)
    rep.kappa('out', gpu[0], cpu16[0], cpu1[0], truth[0], 'out')
    for tag, sel_u, sel_i in (('regular rows', ~urow, ~zero), ('rows at a clamped norm', urow, zero)):
        rep.kappa(f'dU ({tag})', gpu[1][sel_u], cpu16[1][sel_u], cpu1[1][sel_u], truth[1][sel_u], 'dU')
        rep.kappa(f'dI ({tag})', gpu[2][sel_i], cpu16[2][sel_i], cpu1[2][sel_i], truth[2][sel_i], 'dI')
    floored = truth[0] == mu
    assert bool((gpu[0][floored] == np.float32(mu)).all()) and bool((gpu[2][floored] == 0).all()), 'a floored entry is not mu / passes gradient'
    if mu < 0:
        assert float(truth[1][7].abs().max()) > 1e6                  # the clamp gradient really is exercised
    rep.finish()


def test_score_cos_unaligned_and_wide_rows():
    """the scalar path (misaligned pointers with D % 4 == 0) and the re-reading kernels (D > 1024) give the vector path's values"""
    ops = S().ops
    for D in (64, 1100):
        g_ = torch.Generator().manual_seed(1)
        B, N = 33, 3
        u, i, g = torch.randn(B, D, generator=g_), torch.randn(B, N, D, generator=g_), torch.randn(B, N, generator=g_)
        truth = _cos_cpu(u, i, g, 1e-6, torch.float64)
        flat_u, flat_i = torch.zeros(B * D + 1, device=DEV), torch.zeros(B * N * D + 1, device=DEV)
        ud, idv = flat_u[1:].view(B, D), flat_i[1:].view(B, N, D)
        ud.copy_(u), idv.copy_(i)
        assert ud.data_ptr() % 16 != 0 and ud.is_contiguous()
        ud, idv = ud.detach().requires_grad_(True), idv.detach().requires_grad_(True)
        out = ops.ScoreCosFn.apply(ud, idv, 1e-6)
        out.backward(g.to(DEV))
        for got, ref, what in ((out, truth[0], 'out'), (ud.grad, truth[1], 'dU'), (idv.grad, truth[2], 'dI')):
            close(got.detach().cpu(), ref, what=f'D={D} {what}', rtol=1e-5, atol=1e-6)


def test_floor_scores_in_place():
    x = torch.randn(37, 50, device=DEV)
    x[3, 4], x[5, 6] = float('nan'), -float('inf')
    view = x[:, :41]
    ref = evalk_ref.floor_ref(view.cpu(), 0.1).to(DEV)
    keep = x[:, 41:].clone()
    S().ops.floor_scores_(view, 0.1)
    assert torch.equal(view.nan_to_num(7.0), ref.nan_to_num(7.0)) and bool(torch.isnan(view[3, 4])) and float(view[5, 6]) == np.float32(0.1)
    assert torch.equal(x[:, 41:], keep)


# ---- 3. the model against float64 at the ML-1M shape --------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ml1m():
    ds = S().SyntheticDataset(5816, 3299, 651034, seed=0, n_negative_samples=3, holdout_per_user=2, item_popularity=1.0)
    torch.manual_seed(5)
    net = S().DeepMatrixFactorization(ds, [128], [128], 64).to(DEV)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if k.endswith('bias'):
                p.copy_(torch.randn_like(p) * 0.05)
    return ds, net


def _oracle_step(sd_src, ds, batch, kind, dtype):
    sd = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in sd_src.items()}
    u, i, labels = batch
    logits = deepmf_ref.forward(sd, ds.user_sampling_matrix_train, ds.item_sampling_matrix_train, u.numpy(), i.numpy(), mu=1e-6)
    loss = losses_ref.RefRecLoss(kind, n_items=ds.n_items, aggregator='mean', train_neg_strategy='uniform_recbole',
                                 neg_train=3).compute_loss(logits, labels)
    loss.backward()
    return loss.detach().double().reshape(1), {k: v.grad for k, v in sd.items()}


@pytest.mark.parametrize('B', [256, 4096])
def test_deepmf_step_at_ml1m_shape_against_float64(ml1m, B):
    """5,816 users x 3,299 items with long-tailed interactions, towers [., 128, 64]: BCE and BPR loss and every gradient under the three-way
    criterion; then one real AdamW step through Trainer.train_step against the update rule in float64 on the step's own gradients."""
    ds, net = ml1m
    net.train()
    np.random.seed(B)
    batch = next(iter(S().NegativeSamplingDataLoader(ds, batch_size=B, shuffle=True)))
    sd0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    rep = Report(f'DeepMF ML-1M shape B={B}')
    grads = {}
    for kind in ('bce', 'bpr'):
        truth = _oracle_step(sd0, ds, batch, kind, torch.float64)
        cpu16 = _with_threads(16, lambda: _oracle_step(sd0, ds, batch, kind, torch.float32))
        cpu1 = _with_threads(1, lambda: _oracle_step(sd0, ds, batch, kind, torch.float32))
        net.zero_grad()
        u, i, labels = (t.to(DEV) for t in batch)
        loss = _loss(kind, ds.n_items).compute_loss(net(u, i), labels)
        loss.backward()
        rep.kappa(f'{kind} loss', loss.detach().cpu().reshape(1), cpu16[0], cpu1[0], truth[0])
        for k, p in net.named_parameters():
            rep.kappa(f'{kind} grad {k}', p.grad.cpu(), cpu16[1][k], cpu1[1][k], truth[1][k], f'grad {k}')
        grads[kind] = {k: p.grad.detach().cpu().double().clone() for k, p in net.named_parameters()}
    rep.finish()
    # one AdamW step (lr 1e-3, wd 1e-2; step 1: m_hat = g, v_hat = g^2): theta' = theta (1 - lr wd) - lr g / (|g| + eps), in float64, on
    # the step's own gradient. Where |g| is of the order of eps the step moves by lr * dg / eps for a gradient change dg, so the gradient
    # must be THE step's, bit for bit: both passes run in deterministic mode (users repeat within a batch, and outside the mode the
    # per-entity sums of the layer-0 weight gradient add in arrival order).
    ops = S().ops
    prev = ops.set_deterministic(True)
    try:
        net.zero_grad(set_to_none=True)
        u, i, labels = (t.to(DEV) for t in batch)
        _loss('bce', ds.n_items).compute_loss(net(u, i), labels).backward()
        g_step = {k: p.grad.detach().cpu().double().clone() for k, p in net.named_parameters()}
        net.zero_grad(set_to_none=True)
        lr, wd = 1e-3, 1e-2
        conf = {'learn': {'lr': lr, 'wd': wd, 'optimizer': 'adamw'}, 'run_settings': {'device': DEV}}
        tr = S().Trainer(net, None, None, _loss('bce', ds.n_items), conf)
        tr.train_step(*batch)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(prev)
    for k, p in net.named_parameters():
        p0, g = sd0[k].cpu().double(), g_step[k]
        want = p0 * (1 - lr * wd) - lr * g / (g.abs() + 1e-8)
        err = (p.detach().cpu().double() - want).abs()
        # fp32 arithmetic of the update (two moment updates, two bias corrections, square root, sum, quotient, decay, difference: each within
        # one unit roundoff): 16 units in the last place of the larger of the parameter and the lr-sized step
        bound = 16 * 2.0 ** -24 * torch.maximum(p0.abs(), torch.full_like(p0, lr))
        worst = int((err - bound).argmax())
        assert bool((err <= bound).all()), f'AdamW step of {k}: error {float(err.flatten()[worst]):.3e} over {float(bound.flatten()[worst]):.3e}'
    net.load_state_dict(sd0)


# ---- 4. evaluation on all three scorer routes ---------------------------------------------------------------------------------------
ROUTE_C = {'fp32': 72.0, 'fp32_fused': 72.0, 'fp16_fused': 2.0 ** 14 + 72.0}
"""Tolerance of one listed score against the float64 cosine: C * 2^-24 * sum_d |u_d i_d| over the float64-normalised rows. fp32 routes:
scorer_truth_util's C = 64 for the product, plus 8 for the fp32 normalisation of both operands (sum, sqrt, reciprocal, product: <= 4
roundings each). fp16 route: both operands are rounded to fp16 (unit roundoff 2^-11 each: 2^-10 per product = 2^14 * 2^-24) on top."""


class _EvalWorld:
    def __init__(self, n_items_split=None, mu=1e-6, item_scale=False, keep_above=None, train_steps=0):
        """``keep_above`` = n: every user keeps at most n non-excluded items whose float64 cosine is above mu (the others are added to
        its exclusions), so that fewer than k scores above the floor remain whatever the model's cosines look like."""
        Sm = S()
        self.ds = Sm.SyntheticDataset(2000, 3000, 60000, seed=4, n_negative_samples=3, holdout_per_user=1)
        torch.manual_seed(11)
        self.net = Sm.DeepMatrixFactorization(self.ds, [96], [96], 64, mu=mu).to(DEV)
        if train_steps:
            np.random.seed(5)
            tr = Sm.Trainer(self.net, None, None, _loss('bce', 3000), {'learn': {'lr': 2e-3, 'wd': 0., 'optimizer': 'adam'},
                                                                         'run_settings': {'device': DEV}})
            self.net.train()
            ld = Sm.NegativeSamplingDataLoader(self.ds, batch_size=512, shuffle=True)
            it = iter(ld)
            for _ in range(train_steps):
                try:
                    b_ = next(it)
                except StopIteration:
                    it = iter(ld)
                    b_ = next(it)
                tr.train_step(*b_)
        self.net.eval()
        if item_scale:                                             # very unequal item norms: the cosine ignores them, a dot product does not
            scale = torch.logspace(0, 3, 3000, device=DEV)[torch.randperm(3000, generator=torch.Generator().manual_seed(2)).to(DEV)]
            plain = self.net.get_item_representations
            self.net.get_item_representations = lambda idx: plain(idx) * scale[idx.long()][..., None]
        self.view = self.ds.eval_view()
        rng = np.random.default_rng(9)
        if n_items_split is not None:
            self.view.items_in_split = np.sort(rng.choice(3000, size=n_items_split, replace=False))
            self.view.n_items_in_split = n_items_split
        self.items = np.asarray(self.view.items_in_split)
        with torch.no_grad():
            u = self.net.get_user_representations(torch.arange(2000, device=DEV)).double()
            i = self.net.get_item_representations(torch.from_numpy(self.items).to(DEV)).double()
        self.u_raw, self.i_raw = u, i
        self.un = u / u.norm(dim=1, keepdim=True).clamp(min=1e-8)
        self.inn = i / i.norm(dim=1, keepdim=True).clamp(min=1e-8)
        self.cos = self.un @ self.inn.t()
        self.mag = self.un.abs() @ self.inn.abs().t()
        # exclude_data of an evaluation split has the split's items as its columns (data/dataset.py:416-438)
        excluded = torch.from_numpy(T.excl(2000, 3000, 25, seed=3)[0][:, self.items].toarray() != 0).to(DEV)
        if keep_above is not None:
            above = (self.cos > mu) & ~excluded
            excluded |= above & (above.cumsum(1) > keep_above)
        self.excluded = excluded
        import scipy.sparse as sp
        m = sp.csr_matrix(excluded.cpu().numpy())
        m.sort_indices()
        self.view.exclude_data = m
        self.cos_masked = self.cos.masked_fill(self.excluded, -float('inf'))

    def lists(self, scorer, top_k=(1, 10, 20)):
        Sm = S()
        ev = Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=top_k), dataset=self.view)
        got = []
        loader = type('L', (), {'dataset': self.view, 'batch_size': 512})()
        Sm.evaluation._score_split(self.net, loader, ev, DEV, scorer, None, False, 32, lambda s, u_, v, ix: got.append((v, ix)))
        return (torch.cat([g[0] for g in got]), torch.cat([g[1] for g in got])), ev.get_results()


@pytest.fixture(scope='module')
def eval_world():
    return _EvalWorld()


@pytest.mark.parametrize('scorer', ['fp32', 'fp16_fused', 'fp32_fused'])
def test_deepmf_evaluation_lists_against_float64_cosine(eval_world, scorer):
    """2,000 users x 3,000 items, D = 64, random exclusions, top-20: lists and values of every route against the float64 cosine with the
    near-tie acceptance of tests/scorer_truth_util.py (the routes' metrics are compared in the next test)."""
    w = eval_world
    k = 20
    kth = torch.topk(w.cos_masked, k, dim=1).values[:, -1]
    assert bool((kth > w.net.mu).all()), 'condition on the inputs: no tie at the floor reaches a list'
    got, _ = w.lists(scorer)
    rows = torch.arange(2000, device=DEV)
    T.check_against_truth(got, rows, w.cos_masked, ROUTE_C[scorer] * 2.0 ** -24 * w.mag, k, what=scorer)


def _eval(alg, view, scorer, top_k=(1, 10, 20)):
    ev = S().FullEvaluator(config=S().evaluation._Cfg(top_k=top_k, calculate_std=False), dataset=view)
    loader = type('L', (), {'dataset': view, 'batch_size': 64})()
    return S().evaluate_recommender_algorithm(alg, loader, ev, DEV, return_raw=True, scorer=scorer)


def test_deepmf_fused_metrics_match_the_fp32_route(eval_world):
    """The bounds of the existing scorer tests on the 2,000 x 3,000 world (k-th best cosine above mu for every user, asserted: no tie at
    the floor, whose order is unspecified, reaches a list). fp32_fused: the fp32 route's per-user metrics except for at most 3 near-tie
    users (tests/test_hip_scorer_f32.py, unrounded representations). fp16_fused: the mean metrics within 1 % plus two users' hits —
    tests/test_hip_pinned.py allows 1 % + 1e-4 at 20,000 users, where one user's hit is 5e-5 of a mean; here it is 1 / 2,000.
    (A briefly trained DeepMF was tried for this test and is no use: BCE on the floored cosine drives nearly every score to the floor
    within 300 steps, so every list is a tie at mu.)"""
    w = eval_world
    kth = torch.topk(w.cos_masked, 20, dim=1).values[:, -1]
    assert bool((kth > w.net.mu).all()), 'condition on the inputs: no tie at the floor reaches a list'
    (m32, r32), (mf, rf), (mh, _) = (_eval(w.net, w.view, sc) for sc in ('fp32', 'fp32_fused', 'fp16_fused'))
    print('DeepMF metrics (fp32 route):', {k: round(v, 5) for k, v in m32.items()})
    assert m32['ndcg@10'] > 0
    assert list(m32) == list(mf) == list(mh)
    for k in r32:
        n_diff = int((r32[k] != rf[k]).sum())
        assert n_diff <= 3, f'fp32_fused: per-user {k} differs for {n_diff} users'
    for k in m32:
        assert abs(m32[k] - mf[k]) <= 3 / 2000 + 1e-9, (k, m32[k], mf[k])
    for k in ('ndcg@10', 'recall@10', 'precision@10', 'ndcg@20'):
        assert abs(m32[k] - mh[k]) <= 1e-2 * m32[k] + 2 / 2000, (k, m32[k], mh[k])


@pytest.mark.parametrize('scorer', ['fp32', 'fp16_fused', 'fp32_fused'])
def test_deepmf_evaluation_with_the_floor_inside_the_lists(scorer):
    """mu = 0.2 on a 300-item split whose exclusions leave every user at most 7 cosines above the floor, so floored entries reach every list. The values
    equal the floored truth on every route, every item whose cosine is clearly above mu is listed; the order AT the floor is unspecified."""
    w = _EvalWorld(n_items_split=300, mu=0.2, keep_above=7)
    k, mu = 20, 0.2
    (val, idx), _ = w.lists(scorer)
    tol = ROUTE_C[scorer] * 2.0 ** -24 * w.mag
    above = (w.cos_masked > mu).sum(1)
    print(f'{scorer}: {int((above < k).sum())} lists reach the floor, {int((above > 0).sum())} have entries above it')
    assert bool((above < k).all()) and bool(((~w.excluded).sum(1) >= k).all()), 'the floor must reach every list'
    assert bool((idx >= 0).all())
    picked = w.cos_masked.gather(1, idx.long())
    assert bool((picked > -float('inf')).all()), 'an excluded item was listed'
    want = picked.clamp(min=mu)
    err = (val.double() - want).abs()
    assert bool((err <= tol.gather(1, idx.long()) + 2.0 ** -24).all()), f'values differ from the floored truth by {float(err.max())}'
    assert bool((val >= np.float32(mu)).all())
    listed = torch.zeros_like(w.cos_masked, dtype=torch.bool).scatter_(1, idx.long(), True)
    kth = torch.topk(w.cos_masked, k, dim=1).values[:, -1:]
    must = (w.cos_masked > mu + 2 * tol) & (w.cos_masked > kth + 2 * tol)
    assert bool(listed[must].all()), 'an item clearly above the floor and inside the top-k is missing'


def test_fused_lists_rank_by_cosine_not_by_dot_product():
    """Wrong without the model's fused_score_transform: with item norms spread over three decades the fp16_fused lists follow the
    cosine and differ from the plain dot-product ranking of the un-normalised representations."""
    w = _EvalWorld(item_scale=True)
    (val, idx), _ = w.lists('fp16_fused', top_k=(10,))
    dot_rank = torch.topk((w.u_raw @ w.i_raw.t()).masked_fill(w.excluded, -float('inf')), 10, dim=1).indices
    cos_rank = torch.topk(w.cos_masked, 10, dim=1).indices
    differs = (idx.long() != dot_rank).any(1)
    assert int(differs.sum()) >= 1, 'the fused route ranks by the raw dot product'
    assert float((idx.long()[:, 0] == cos_rank[:, 0]).double().mean()) > 0.8
    assert float((dot_rank[:, 0] == cos_rank[:, 0]).double().mean()) < 0.5
    assert bool((val <= 1.0 + 1e-3).all())


# ---- 5. deterministic mode ----------------------------------------------------------------------------------------------------------------
def _train_50(seed, final=64):
    Sm = S()
    Sm.reproducible(seed)
    ds = Sm.SyntheticDataset(400, 300, 9000, seed=1, n_negative_samples=3)
    net = Sm.DeepMatrixFactorization(ds, [32], [32], final, normalize_representations=True)
    conf = {'learn': {'lr': 1e-3, 'wd': 1e-4, 'optimizer': 'adamw'}, 'run_settings': {'device': DEV}}
    tr = Sm.Trainer(net, None, None, _loss('bce', 300), conf)
    net.train()
    ld = Sm.NegativeSamplingDataLoader(ds, batch_size=64, shuffle=True)
    it = iter(ld)
    for _ in range(50):
        try:
            b = next(it)
        except StopIteration:
            it = iter(ld)
            b = next(it)
        tr.train_step(*b)
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def test_deepmf_deterministic_training_is_bit_identical():
    ops = S().ops
    prev = ops.is_deterministic()
    try:
        ops.nondeterministic_launches(reset=True)
        a = _train_50(123)
        b = _train_50(123)
        assert ops.nondeterministic_launches() == 0
        assert ops.is_deterministic()
        for k in a:
            assert torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)), k
    finally:
        ops.set_deterministic(prev)


def test_deepmf_deterministic_mode_refuses_the_scatter_form():
    """a layer-0 width with C % 4 != 0 has no gather-form weight gradient: deterministic mode raises instead of running the atomics"""
    Sm = S()
    prev = Sm.ops.is_deterministic()
    try:
        Sm.ops.set_deterministic(True)
        ds = Sm.SyntheticDataset(100, 80, 1500, seed=1, n_negative_samples=3)
        net = Sm.DeepMatrixFactorization(ds, [], [], 5).to(DEV).train()
        u, i = torch.arange(8, device=DEV), torch.randint(0, 80, (8, 4), device=DEV)
        with pytest.raises(Sm.SibrarHipError, match='no deterministic form'):
            net(u, i).sum().backward()
        Sm.ops.set_deterministic(False)
        net.zero_grad()
        net(u, i).sum().backward()                                     # the scatter form serves it outside the mode
        assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    finally:
        Sm.ops.set_deterministic(prev)


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------------
def test_deepmf_fit_and_checkpoint_round_trip(tmp_path):
    Sm = S()
    torch.manual_seed(0)
    np.random.seed(0)
    ds = Sm.SyntheticDataset(500, 300, 15000, seed=2, n_negative_samples=4, holdout_per_user=1)
    net = Sm.ALGORITHMS['dmf'].build_from_conf({'u_mid_layers': [64], 'i_mid_layers': [64], 'final_dimension': 32}, ds)
    loader = Sm.NegativeSamplingDataLoader(ds, batch_size=256, shuffle=True)
    val = type('L', (), {'dataset': ds.eval_view(), 'batch_size': 256})()
    conf = {'learn': {'lr': 1e-3, 'wd': 0., 'optimizer': 'adam', 'n_epochs': 2}, 'run_settings': {'device': DEV},
            'eval': Sm.evaluation._Cfg(top_k=(10,)), 'results_path': str(tmp_path)}
    tr = Sm.Trainer(net, loader, val, _loss('bce', 300, 4), conf)
    first = tr.train()['train/loss']
    best = tr.fit()
    last = tr.train()['train/loss']
    assert last < first, (first, last)
    assert np.isfinite(best['ndcg@10']) and 0.0 <= best['ndcg@10'] <= 1.0
    net.save_model_to_path(str(tmp_path))
    other = Sm.ALGORITHMS['dmf'].build_from_conf({'u_mid_layers': [64], 'i_mid_layers': [64], 'final_dimension': 32}, ds).to(DEV)
    other.load_model_from_path(str(tmp_path))
    for (k, a), (_, b) in zip(net.state_dict().items(), other.state_dict().items()):
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), k
