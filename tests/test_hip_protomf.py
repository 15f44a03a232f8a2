"""ProtoMF (uprotomf, iprotomf, uiprotomf) on the GPU: the product classes against the G18 fixture of the real reference, the fused
similarity kernels and the whole models against float64 under the three-way criterion of tests/test_hip_c1.py and tests/test_hip_deepmf.py

    err(GPU, truth) <= KAPPA * max(err(torch-CPU fp32, 16 threads), err(torch-CPU fp32, 1 thread)) + REL_FLOOR * ||truth||

(err = 2-norm of the difference per tensor; KAPPA and REL_FLOOR are those files' values; the measured ratios are printed), full-catalogue
evaluation on all three scorer routes, the deterministic mode, and one end-to-end fit. Inputs whose arg-mins could flip between fp32 and
float64 are constructed away (tests/protomf_inputs.py) and the precondition is asserted in float64 before anything is compared."""
import json
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import protomf_inputs
import protomf_ref
from golden_util import GOLDEN, I, close, host_dataset, load, state_dict, world
from oracle import losses_ref
import scorer_truth_util as T

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = dict(rtol=1e-4, atol=1e-5)                                 # tests/test_hip_deepmf.py
CASES = json.load(open(os.path.join(GOLDEN, 'g18_protomf.json')))['cases']
KAPPA = 3.0                                                      # tests/test_hip_c1.py, tests/test_hip_deepmf.py
REL_FLOOR = 1e-7
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
def test_g18_protomf_on_hip_kernels(case):
    """The product classes == the real reference on every G18 case: train-mode logits, every loss-dictionary entry, BCE and BPR loss,
    every gradient of rec_loss + reg_loss under each loss, evaluation scores through get_*_representations + combine, post_val."""
    z = load('g18_protomf')
    name = case['name']
    m = S().ALGORITHMS[case['alg']].build_from_conf(case['conf'], host_dataset(world(z)))
    sd = state_dict(z, f'{name}/sd/')
    assert list(m.state_dict().keys()) == list(sd.keys()) == case['keys']
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
        assert list(other) == case['other_keys']
        for k, v in other.items():
            assert v.is_cuda, f'{k} left the device'
            close(v.detach().cpu(), z[f'{name}/other_{kind}/{k}'], what=f'{kind} {k}', **TOL)
        (loss + other['reg_loss']).backward()
        for k, p in m.named_parameters():
            close(p.grad.cpu(), z[f'{name}/grad_{kind}/{k}'], what=f'{kind} grad {k}', rtol=1e-4, atol=1e-6, norm_rtol=1e-4)
    m.eval()
    with torch.no_grad():
        ir = m.get_item_representations(torch.arange(I, device=DEV))
        scores = m.combine_user_item_representations(m.get_user_representations(u), ir)
    close(scores.cpu(), z[f'{name}/scores_all'], what='all-pairs scores', **TOL)
    pv = m.post_val(0)
    assert list(pv) == list(case['post_val']) and all(isinstance(v, float) for v in pv.values())
    for k, v in pv.items():
        close(torch.tensor(v), torch.tensor(case['post_val'][k]), what=f'post_val {k}', **TOL)


# ---- 2. the kernels against float64 -------------------------------------------------------------------------------------------------
W_PROTO, W_BATCH = 0.7, 1.3                                      # regulariser weights of the kernel tests (unequal, both of order 1)


def _sim_cpu(e, protos, G, dtype):
    """(sim, proto_loss, batch_loss, dE, dP) of sum(sim * G) + W_PROTO proto_loss + W_BATCH batch_loss by torch autograd"""
    e, p = e.to(dtype).clone().requires_grad_(True), protos.to(dtype).clone().requires_grad_(True)
    sim = protomf_ref.shifted_cosine_sim(e, p)
    pl, bl = protomf_ref.reg_losses(sim)
    ((sim * G.to(dtype)).sum() + W_PROTO * pl + W_BATCH * bl).backward()
    return sim.detach(), pl.detach().reshape(1), bl.detach().reshape(1), e.grad, p.grad


def _sim_gpu(table, rows, protos, G):
    t, p = table.to(DEV).requires_grad_(True), protos.to(DEV).requires_grad_(True)
    sim, pl, bl = S().ops.ProtoSimFn.apply(t, rows.to(DEV), p)
    ((sim * G.to(DEV)).sum() + W_PROTO * pl + W_BATCH * bl).backward()
    torch.cuda.synchronize()
    return sim.detach().cpu(), pl.detach().cpu().reshape(1), bl.detach().cpu().reshape(1), t.grad.cpu(), p.grad.cpu()


def _assert_margins(e, protos):
    row_m, col_m = protomf_inputs.margins(e.double(), protos.double())
    if e.shape[1] == 1:
        assert protomf_inputs.exact_only(row_m) and protomf_inputs.exact_only(col_m), 'D = 1: margins are exactly 0 or 2'
    else:
        assert float(row_m.min()) >= protomf_inputs.MARGIN and float(col_m.min()) >= protomf_inputs.MARGIN, 'precondition: arg-min margins'


@pytest.mark.parametrize('R,D,P', [(37, 100, 20), (45056, 100, 20), (32768, 128, 64), (8192, 64, 128), (4096, 512, 256), (3, 1, 2)])
def test_proto_sim_kernels_against_float64(R, D, P):
    """sim, both losses, dE and dP of ops.ProtoSimFn against torch autograd in float64. The rows are a permutation of the table, so dE is
    the table gradient read back through the lookup. (3, 1, 2): every similarity is exactly 0 or 2 and every gradient exactly 0, in every
    precision — the comparison then asks for exact zeros, ties included."""
    table, rows, protos = protomf_inputs.argmin_safe(R, D, P, seed=R + D + P)
    e = table[rows.long()]
    _assert_margins(e, protos)
    G = torch.randn(R, P, generator=torch.Generator().manual_seed(R)) / R
    truth = _sim_cpu(e, protos, G, torch.float64)
    cpu16 = _with_threads(16, lambda: _sim_cpu(e, protos, G, torch.float32))
    cpu1 = _with_threads(1, lambda: _sim_cpu(e, protos, G, torch.float32))
    gpu = _sim_gpu(table, rows, protos, G)
    gpu = gpu[:3] + (gpu[3][rows.long()], gpu[4])
    rep = Report(f'proto_sim R={R} D={D} P={P}')
    for n, what in enumerate(('sim', 'proto_loss', 'batch_loss', 'dE', 'dP')):
        rep.kappa(what, gpu[n], cpu16[n], cpu1[n], truth[n])
    rep.finish()


def test_proto_sim_duplicate_rows_at_the_table_gradient():
    """A batch that names table rows several times: identical rows tie exactly in every minimum; whichever of them takes the regulariser's
    gradient, the scattered TABLE gradient is the same, so that is what is compared (the distinct rows are arg-min safe)."""
    n_table, R, D, P = 300, 4096, 100, 20
    table, _, protos = protomf_inputs.argmin_safe(n_table, D, P, seed=77)
    gen = torch.Generator().manual_seed(78)
    rows = torch.cat([torch.arange(n_table), torch.randint(0, n_table, (R - n_table,), generator=gen)])[torch.randperm(R, generator=gen)].to(torch.int32)
    _assert_margins(table, protos)
    G = torch.randn(R, P, generator=gen) / R

    def cpu(dtype):
        t, p = table.to(dtype).clone().requires_grad_(True), protos.to(dtype).clone().requires_grad_(True)
        sim = protomf_ref.shifted_cosine_sim(t[rows.long()], p)
        pl, bl = protomf_ref.reg_losses(sim)
        ((sim * G.to(dtype)).sum() + W_PROTO * pl + W_BATCH * bl).backward()
        return sim.detach(), pl.detach().reshape(1), bl.detach().reshape(1), t.grad, p.grad

    truth, cpu16, cpu1 = cpu(torch.float64), _with_threads(16, lambda: cpu(torch.float32)), _with_threads(1, lambda: cpu(torch.float32))
    gpu = _sim_gpu(table, rows, protos, G)
    rep = Report('proto_sim with duplicate rows')
    for n, what in enumerate(('sim', 'proto_loss', 'batch_loss', 'd table', 'dP')):
        rep.kappa(what, gpu[n], cpu16[n], cpu1[n], truth[n])
    rep.finish()


def test_proto_sim_colinear_rows_stay_in_range():
    """forward only: rows that are positive / negative multiples of a prototype give similarities in [0, 2], within 1e-6 of 2 / 0"""
    gen = torch.Generator().manual_seed(3)
    for D, P in ((100, 20), (128, 64), (7, 3)):
        protos = torch.randn(P, D, generator=gen)
        scale = torch.logspace(-3, 3, P).unsqueeze(1)
        table = torch.cat([protos * scale, -protos * scale]).to(DEV)
        sim = S().ops.proto_sim(table, None, protos.to(DEV)).cpu()
        assert bool((sim >= 0).all()) and bool((sim <= 2).all())
        d = torch.arange(P)
        assert float((sim[d, d] - 2).abs().max()) <= 1e-6 and float(sim[P + d, d].abs().max()) <= 1e-6
        sim_t, _, _ = S().ops.ProtoSimFn.apply(table, torch.arange(2 * P, device=DEV), protos.to(DEV))
        assert torch.equal(sim_t.cpu(), sim)


def test_proto_sim_shapes_outside_the_range_raise():
    ops = S().ops
    for D, P in ((513, 20), (100, 1), (100, 257)):
        with pytest.raises(ValueError, match='n_prototypes'):
            ops.proto_sim(torch.zeros(3, D, device=DEV), None, torch.zeros(P, D, device=DEV))
    L = import_module(ops.__name__.rsplit('.', 1)[0] + '._lib')
    x = torch.zeros(4, 8, device=DEV)
    with pytest.raises(S().SibrarHipError, match='n_proto'):           # the entry point itself refuses through sbr_last_error
        L.call('sbr_proto_sim_fwd', x.data_ptr(), 8, None, 4, 8, x.data_ptr(), 1, x.data_ptr(), None, None, None, None, None, None, None,
               None, x.data_ptr(), 0, L.stream())
    empty = ops.proto_sim(x, torch.zeros(0, dtype=torch.long, device=DEV), x)
    assert tuple(empty.shape) == (0, 4)


# ---- 3. the models against float64 at the ML-1M shape -------------------------------------------------------------------------------
MODEL_CONFS = [
    ('uprotomf', dict(embedding_dim=100, n_prototypes=20, sim_proto_weight=1., sim_batch_weight=1.)),
    ('iprotomf', dict(embedding_dim=100, n_prototypes=20, sim_proto_weight=1., sim_batch_weight=1.)),
    ('uiprotomf', dict(embedding_dim=100, u_n_prototypes=20, i_n_prototypes=20, u_sim_proto_weight=1., u_sim_batch_weight=1.,
                       i_sim_proto_weight=1., i_sim_batch_weight=1.)),
    ('uprotomf', dict(embedding_dim=128, n_prototypes=64, sim_proto_weight=1., sim_batch_weight=1.)),
]


@pytest.fixture(scope='module')
def ml1m_ds():
    return S().SyntheticDataset(5816, 3299, 651034, seed=0, n_negative_samples=3, holdout_per_user=2, item_popularity=1.0)


def _sides(alg, sd):
    """(table key, prototypes key, 'user' | 'item') of every prototype side of a model"""
    if alg == 'uiprotomf':
        return [('uprotomf.user_embed.weight', 'uprotomf.prototypes', 'user'), ('iprotomf.item_embed.weight', 'iprotomf.prototypes', 'item')]
    return [('user_embed.weight', 'prototypes', 'user')] if alg == 'uprotomf' else [('item_embed.weight', 'prototypes', 'item')]


def _oracle_step(alg, conf, sd_src, batch, kind, n_items, dtype):
    sd = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in sd_src.items()}
    u, i, labels = batch
    logits, other = protomf_ref.forward(alg, sd, conf, u, i)
    loss = losses_ref.RefRecLoss(kind, n_items=n_items, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=3).compute_loss(logits, labels)
    (loss + other['reg_loss']).backward()
    out = {'logits': logits.detach(), 'loss': loss.detach().double().reshape(1)}
    out.update({f'other {k}': v.detach().reshape(1) for k, v in other.items()})
    return out, {k: v.grad for k, v in sd.items()}


@pytest.mark.parametrize('alg,conf', MODEL_CONFS, ids=lambda v: v if isinstance(v, str) else f'{v["embedding_dim"]}')
def test_protomf_step_at_ml1m_shape_against_float64(ml1m_ds, alg, conf):
    """5,816 users x 3,299 items, one batch of 4,096 users with 1 + 3 items each: logits, BCE and BPR loss, every loss-dictionary entry
    and every gradient of rec_loss + reg_loss under the three-way criterion. The embeddings are drawn at unit scale (at the initial
    0.1 / dim every gradient carries a factor 1 / |e| of 1e2 .. 1e3 and nothing else is visible) and made arg-min safe on the batch."""
    ds = ml1m_ds
    torch.manual_seed(5)
    net = S().ALGORITHMS[alg].build_from_conf(conf, ds)
    np.random.seed(4096)
    batch = next(iter(S().NegativeSamplingDataLoader(ds, batch_size=4096, shuffle=True)))
    gen = torch.Generator().manual_seed(6)
    sd0 = {k: torch.randn(v.shape, generator=gen) * 0.5 for k, v in net.state_dict().items()}
    for t_key, p_key, side in _sides(alg, sd0):
        used = torch.unique(batch[0] if side == 'user' else batch[1])
        protomf_inputs.make_safe(sd0[t_key], used, sd0[p_key], gen, 0.5)
        row_m, col_m = protomf_inputs.margins(sd0[t_key][used].double(), sd0[p_key].double())
        assert float(row_m.min()) >= protomf_inputs.MARGIN and float(col_m.min()) >= protomf_inputs.MARGIN, 'precondition: arg-min margins'
    net.load_state_dict(sd0)
    net.to(DEV).train()
    rep = Report(f'{alg} {conf} at the ML-1M shape')
    for kind in ('bce', 'bpr'):
        truth = _oracle_step(alg, conf, sd0, batch, kind, ds.n_items, torch.float64)
        cpu16 = _with_threads(16, lambda: _oracle_step(alg, conf, sd0, batch, kind, ds.n_items, torch.float32))
        cpu1 = _with_threads(1, lambda: _oracle_step(alg, conf, sd0, batch, kind, ds.n_items, torch.float32))
        net.zero_grad()
        u, i, labels = (t.to(DEV) for t in batch)
        logits = net(u, i)
        loss = _loss(kind, ds.n_items).compute_loss(logits, labels)
        other = net.get_and_reset_other_loss()
        (loss + other['reg_loss']).backward()
        got = {'logits': logits.detach().cpu(), 'loss': loss.detach().cpu().reshape(1)}
        got.update({f'other {k}': v.detach().cpu().reshape(1) for k, v in other.items()})
        assert list(got) == list(truth[0])
        for k in got:
            rep.kappa(f'{kind} {k}', got[k], cpu16[0][k], cpu1[0][k], truth[0][k], k)
        for k, p in net.named_parameters():
            rep.kappa(f'{kind} grad {k}', p.grad.cpu(), cpu16[1][k], cpu1[1][k], truth[1][k], f'grad {k}')
    rep.finish()


# ---- 4. evaluation ----------------------------------------------------------------------------------------------------------------------
ROUTE_C = {'fp32': 72.0, 'fp32_fused': 72.0, 'fp16_fused': 2.0 ** 14 + 72.0}
"""Tolerance of one listed score against float64: C * 2^-24 * sum_d |u_d i_d| (tests/test_hip_deepmf.py): scorer_truth_util's C = 64 for
the product plus 8 for the fp32 similarity operand (values in [0, 2] with a few roundings each); the fp16 route rounds both operands to
fp16 on top (2^-10 per product)."""


class _EvalWorld:
    def __init__(self, alg, conf):
        Sm = S()
        self.ds = Sm.SyntheticDataset(2000, 3000, 60000, seed=4, n_negative_samples=3, holdout_per_user=1)
        torch.manual_seed(11)
        self.alg, self.conf = alg, conf
        self.net = Sm.ALGORITHMS[alg].build_from_conf(conf, self.ds)
        gen = torch.Generator().manual_seed(12)
        self.net.load_state_dict({k: torch.randn(v.shape, generator=gen) * 0.5 for k, v in self.net.state_dict().items()})
        self.net.to(DEV).eval()
        self.view = self.ds.eval_view()
        sd = {k: v.detach().cpu().double() for k, v in self.net.state_dict().items()}
        with torch.no_grad():
            self.u64 = protomf_ref.representations(alg, sd, 'user', torch.arange(2000))
            self.i64 = protomf_ref.representations(alg, sd, 'item', torch.arange(3000))
            self.scores = protomf_ref.combine(alg, self.u64, self.i64).to(DEV)
        self.excluded = torch.from_numpy(self.view.exclude_data.toarray() != 0).to(DEV)
        self.masked = self.scores.masked_fill(self.excluded, -float('inf'))

    def lists(self, scorer, top_k=(1, 10, 20)):
        Sm = S()
        ev = Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=top_k), dataset=self.view)
        got = []
        loader = type('L', (), {'dataset': self.view, 'batch_size': 512})()
        Sm.evaluation._score_split(self.net, loader, ev, DEV, scorer, None, False, 32, lambda s, u_, v, ix: got.append((v, ix)))
        return torch.cat([g[0] for g in got]), torch.cat([g[1] for g in got])


def _eval(alg, view, scorer, top_k=(1, 10, 20)):
    ev = S().FullEvaluator(config=S().evaluation._Cfg(top_k=top_k, calculate_std=False), dataset=view)
    loader = type('L', (), {'dataset': view, 'batch_size': 64})()
    return S().evaluate_recommender_algorithm(alg, loader, ev, DEV, return_raw=True, scorer=scorer)


@pytest.fixture(scope='module')
def eval_world_64():
    return _EvalWorld('uprotomf', dict(embedding_dim=100, n_prototypes=64, sim_proto_weight=1., sim_batch_weight=1.))


@pytest.mark.parametrize('scorer', ['fp32', 'fp16_fused', 'fp32_fused'])
def test_uprotomf_evaluation_lists_against_float64(eval_world_64, scorer):
    """uprotomf with 64 prototypes (representations 64 wide: the fused routes take it), 2,000 users x 3,000 items, top-20 lists of every
    route against the float64 scores' ranking with the near-tie acceptance of tests/scorer_truth_util.py; then the metrics."""
    w = eval_world_64
    L = import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')
    L.CALL_LOG = []
    try:
        got = w.lists(scorer)
        names = {n for n, _ in L.CALL_LOG}
    finally:
        L.CALL_LOG = None
    assert any(n.startswith('sbr_score_topk_f') for n in names) == (scorer != 'fp32'), names
    mag = (w.u64.abs() @ w.i64.abs().t()).to(DEV)
    T.check_against_truth(got, torch.arange(2000, device=DEV), w.masked, ROUTE_C[scorer] * 2.0 ** -24 * mag, 20, what=scorer)
    metrics, _ = _eval(w.net, w.view, scorer)
    assert 0.0 <= metrics['ndcg@10'] <= 1.0


def _metrics_from_scores(view, masked, top_k=(1, 10, 20)):
    ev = S().FullEvaluator(config=S().evaluation._Cfg(top_k=top_k, calculate_std=False), dataset=view)
    idx = torch.topk(masked, max(top_k), dim=1).indices.to(torch.int32)
    ev.eval_topk(torch.arange(masked.shape[0], device=DEV), idx)
    return ev.get_results(return_raw_results=True)


def _same_metrics(got, want, n_users, what):
    """per-user metrics equal except for at most 3 users (near-ties of the fp32 scores in float64, tests/test_hip_deepmf.py)"""
    (m_got, r_got), (m_want, r_want) = got, want
    assert list(m_got) == list(m_want)
    for k in r_want:
        n_diff = int((torch.as_tensor(r_got[k]).cpu() != torch.as_tensor(r_want[k]).cpu()).sum())
        assert n_diff <= 3, f'{what}: per-user {k} differs for {n_diff} users'
    for k in m_want:
        assert abs(m_got[k] - m_want[k]) <= 3 / n_users + 1e-9, (what, k, m_got[k], m_want[k])


def test_uprotomf_default_width_falls_back_to_fp32():
    """n_prototypes = 20: no fused kernel is built for 20-wide representations, so a fused request takes the fp32 route — no fused scorer
    entry point is called and the metrics are the fp32 route's, bit for bit — and they equal the float64 restatement's."""
    w = _EvalWorld('uprotomf', dict(embedding_dim=100, n_prototypes=20, sim_proto_weight=1., sim_batch_weight=1.))
    assert not S().ops.score_topk_fused_supported('fp16_fused', 20, 20) and not S().ops.score_topk_fused_supported('fp32_fused', 20, 20)
    L = import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')
    ref = _eval(w.net, w.view, 'fp32')
    for scorer in ('fp16_fused', 'fp32_fused'):
        L.CALL_LOG = []
        try:
            got = _eval(w.net, w.view, scorer)
            names = {n for n, _ in L.CALL_LOG}
        finally:
            L.CALL_LOG = None
        assert not any(n.startswith('sbr_score_topk_f') for n in names), names
        assert 'sbr_proto_sim_fwd' in names
        assert got[0] == ref[0] and all(torch.equal(torch.as_tensor(got[1][k]), torch.as_tensor(ref[1][k])) for k in ref[1])
    _same_metrics(ref, _metrics_from_scores(w.view, w.masked), 2000, 'uprotomf 20')


def test_uiprotomf_metrics_on_the_fp32_route_equal_the_restatement():
    w = _EvalWorld('uiprotomf', dict(embedding_dim=100, u_n_prototypes=20, i_n_prototypes=12, u_sim_proto_weight=1., u_sim_batch_weight=1.,
                                     i_sim_proto_weight=1., i_sim_batch_weight=1.))
    got = _eval(w.net, w.view, 'fp32')
    print('UIProtoMF metrics (fp32 route):', {k: round(v, 5) for k, v in got[0].items()})
    _same_metrics(got, _metrics_from_scores(w.view, w.masked), 2000, 'uiprotomf')
    fused = _eval(w.net, w.view, 'fp16_fused')                         # a tuple model: the fused request takes the fp32 route
    assert fused[0] == got[0]


# ---- 5. deterministic mode ----------------------------------------------------------------------------------------------------------------
DET_CONFS = {
    'uprotomf': dict(embedding_dim=100, n_prototypes=20, sim_proto_weight=0.5, sim_batch_weight=0.25),
    'uiprotomf': dict(embedding_dim=48, u_n_prototypes=20, i_n_prototypes=12, u_sim_proto_weight=0.5, u_sim_batch_weight=0.25,
                      i_sim_proto_weight=0.125, i_sim_batch_weight=1.),
}


def _train_50(alg, seed):
    Sm = S()
    Sm.reproducible(seed)
    ds = Sm.SyntheticDataset(400, 300, 9000, seed=1, n_negative_samples=3)
    net = Sm.ALGORITHMS[alg].build_from_conf(DET_CONFS[alg], ds)
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


@pytest.mark.parametrize('alg', ['uprotomf', 'uiprotomf'])
def test_protomf_deterministic_training_is_bit_identical(alg):
    ops = S().ops
    prev = ops.is_deterministic()
    try:
        ops.nondeterministic_launches(reset=True)
        a = _train_50(alg, 123)
        b = _train_50(alg, 123)
        assert ops.nondeterministic_launches() == 0
        assert ops.is_deterministic()
        for k in a:
            assert torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)), k
        assert any(not torch.equal(a[k], torch.zeros_like(a[k])) for k in a)
    finally:
        ops.set_deterministic(prev)


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alg', ['uprotomf', 'iprotomf', 'uiprotomf'])
def test_protomf_fit_and_checkpoint_round_trip(tmp_path, alg):
    Sm = S()
    torch.manual_seed(0)
    np.random.seed(0)
    ds = Sm.SyntheticDataset(500, 300, 15000, seed=2, n_negative_samples=4, holdout_per_user=1)
    conf_m = DET_CONFS['uiprotomf'] if alg == 'uiprotomf' else DET_CONFS['uprotomf']
    net = Sm.ALGORITHMS[alg].build_from_conf(conf_m, ds)
    loader = Sm.NegativeSamplingDataLoader(ds, batch_size=256, shuffle=True)
    val = type('L', (), {'dataset': ds.eval_view(), 'batch_size': 256})()
    conf = {'learn': {'lr': 1e-3, 'wd': 0., 'optimizer': 'adam', 'n_epochs': 2}, 'run_settings': {'device': DEV},
            'eval': Sm.evaluation._Cfg(top_k=(10,)), 'results_path': str(tmp_path)}
    tr = Sm.Trainer(net, loader, val, _loss('bce', 300, 4), conf)
    losses = tr.train()
    reg_keys = ['reg_loss', 'proto_loss', 'batch_loss'] if alg != 'uiprotomf' else ['reg_loss', 'user_proto_loss', 'user_batch_loss',
                                                                                     'item_proto_loss', 'item_batch_loss']
    assert list(losses) == ['train/loss', 'train/rec_loss'] + [f'train/{k}' for k in reg_keys]
    assert all(np.isfinite(v) for v in losses.values()) and losses['train/reg_loss'] > 0
    best = tr.fit()
    stats = ('avg_pairwise_proto_sim', 'entity_to_proto_mean', 'entity_to_proto_max', 'entity_to_proto_min')
    pv_keys = list(stats) if alg != 'uiprotomf' else [f'{s}_{k}' for s in ('user', 'item') for k in stats]
    for k in pv_keys:
        assert k in best and isinstance(best[k], float) and 0.0 <= best[k] <= 2.0, (k, best.get(k))
    assert np.isfinite(best['ndcg@10']) and 0.0 <= best['ndcg@10'] <= 1.0
    assert tr.train()['train/loss'] < losses['train/loss']
    net.save_model_to_path(str(tmp_path))
    other = Sm.ALGORITHMS[alg].build_from_conf(conf_m, ds).to(DEV)
    other.load_model_from_path(str(tmp_path))
    for (k, a), (_, b) in zip(net.state_dict().items(), other.state_dict().items()):
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), k
