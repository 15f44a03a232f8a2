"""The simplified ProtoMF models (uprotomfs, iprotomfs, uiprotomfs) on the GPU: the product classes against the G21 fixture of the real
reference, ops.ProtoCosFn / ops.ProtoScoreFn (csrc/proto_cos.hip) and the models against float64 under the three-way criterion of
tests/test_hip_protomf.py (its KAPPA, REL_FLOOR, TOL and Report; the measured ratios are printed), the kinks compared exactly, the fused
route against the composed one, the deterministic mode, full-catalogue evaluation and one end-to-end fit per registry name."""
import json
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import protomfs_ref
import test_hip_protomf as PM
from golden_util import GOLDEN, I, close, host_dataset, load, state_dict, world
import scorer_truth_util as T

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL, Report, _with_threads, _loss, S = PM.TOL, PM.Report, PM._with_threads, PM._loss, PM.S
CASES = json.load(open(os.path.join(GOLDEN, 'g21_protomfs.json')))['cases']
STATS = ('avg_pairwise_proto_sim', 'entity_to_proto_mean', 'entity_to_proto_max', 'entity_to_proto_min', 'bin_weights_mean',
         'sum_weights_mean')


def _three(fn):
    """(float64 truth, torch-CPU fp32 at 16 threads, at 1 thread) of fn(dtype)"""
    return fn(torch.float64), _with_threads(16, lambda: fn(torch.float32)), _with_threads(1, lambda: fn(torch.float32))


# ---- 1. golden parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_g21_protomfs_on_hip_kernels(case):
    """The product classes == the real reference on every G21 case: train-mode logits (the fused route), BCE and BPR loss, every
    gradient under each loss, evaluation scores through get_*_representations + combine (the composed route), post_val."""
    z = load('g21_protomfs')
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
        assert list(m.get_and_reset_other_loss()) == ['reg_loss']
        loss.backward()
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
SHAPES = [(1, 1, 2, 1), (37, 100, 20, 4), (65, 33, 65, 1), (130, 64, 64, 11), (64, 512, 256, 2)]


def _inputs(R, D, P, fan, seed):
    """table (R + 3 rows, the batch a partial permutation of them), prototypes, a weight table of R fan + 2 rows (widx a partial
    permutation) whose entries are exactly 0 (about one in five), or of either sign with |w| >= 1e-3"""
    gen = torch.Generator().manual_seed(seed)
    table, protos = torch.randn(R + 3, D, generator=gen), torch.randn(P, D, generator=gen)
    rows = torch.randperm(R + 3, generator=gen)[:R].to(torch.int32)
    wt = torch.randn(R * fan + 2, P, generator=gen)
    wt = torch.where(wt.abs() < 1e-3, torch.full_like(wt, 1e-3), wt)
    wt[torch.rand(wt.shape, generator=gen) < 0.2] = 0.
    widx = torch.randperm(R * fan + 2, generator=gen)[:R * fan].to(torch.int32)
    return table, rows, protos, wt, widx, gen


def _assert_away_from_kinks(e, protos, w):
    """in float64: every |w| >= 1e-3 or exactly 0; every |cos| <= 1 - 1e-3 — except at D = 1, where every cosine is exactly +-1 in every
    precision (x / |x|), the clamp's closed interval passes the gradient and the normalisation gradient is exactly 0"""
    w = w.double()
    assert bool(((w == 0) | (w.abs() >= 1e-3)).all()), 'precondition: weights at the ReLU kink'
    cos = torch.nn.functional.normalize(e.double()) @ torch.nn.functional.normalize(protos.double()).T
    if e.shape[1] == 1:
        assert bool((cos.abs() == 1).all()), 'D = 1: cosines are exactly +-1'
    else:
        assert float(cos.abs().max()) <= 1 - 1e-3, 'precondition: cosines at the clamp'


def _score_cpu(e, protos, w, G, dtype):
    """(out, dE, dP, dW) of sum(out * G) by torch autograd; w [R, fan, P] are the gathered weight rows"""
    e, p, w = (t.to(dtype).clone().requires_grad_(True) for t in (e, protos, w))
    out = protomfs_ref.score(e, p, w)
    (out * G.to(dtype)).sum().backward()
    return out.detach(), e.grad, p.grad, w.grad


@pytest.mark.parametrize('with_widx', [True, False], ids=['widx', 'rows'])
@pytest.mark.parametrize('R,D,P,fan', SHAPES)
def test_proto_score_kernels_against_float64(R, D, P, fan, with_widx):
    """out, dE, dP and dWeights of ops.ProtoScoreFn against torch autograd in float64, with the weight rows gathered through widx (the
    weight gradient is then the table gradient, read back through the permutation) and given in order (widx None)."""
    table, rows, protos, wt, widx, gen = _inputs(R, D, P, fan, seed=R + D + P + fan)
    e, w = table[rows.long()], wt[widx.long()].reshape(R, fan, P)
    _assert_away_from_kinks(e, protos, w)
    G = torch.randn(R, fan, generator=gen) / R
    truth, cpu16, cpu1 = _three(lambda dt: _score_cpu(e, protos, w, G, dt))
    t, p = table.to(DEV).requires_grad_(True), protos.to(DEV).requires_grad_(True)
    wg = (wt if with_widx else w.reshape(R * fan, P)).to(DEV).requires_grad_(True)
    out = S().ops.ProtoScoreFn.apply(t, rows.to(DEV), p, wg, widx.to(DEV) if with_widx else None, fan)
    assert tuple(out.shape) == (R, fan)
    (out * G.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    dW = wg.grad.cpu()
    if with_widx:
        unused = torch.ones(len(wt), dtype=torch.bool)
        unused[widx.long()] = False
        assert float(dW[unused].abs().max()) == 0., 'weight rows outside widx took a gradient'
        dW = dW[widx.long()]
    gpu = (out.detach().cpu(), t.grad.cpu()[rows.long()], p.grad.cpu(), dW.reshape(R, fan, P))
    rep = Report(f'proto_score R={R} D={D} P={P} fan={fan} widx={with_widx}')
    for n, what in enumerate(('out', 'dE', 'dP', 'dWeights')):
        rep.kappa(what, gpu[n], cpu16[n], cpu1[n], truth[n])
    rep.finish()


def _cos_cpu(e, protos, G, dtype):
    e, p = (t.to(dtype).clone().requires_grad_(True) for t in (e, protos))
    cos = protomfs_ref.cosine_sim(e, p)
    (cos * G.to(dtype)).sum().backward()
    return cos.detach(), e.grad, p.grad


@pytest.mark.parametrize('R,D,P,fan', SHAPES)
def test_proto_cos_kernels_against_float64(R, D, P, fan):
    """cos, dE and dP of ops.ProtoCosFn against torch autograd in float64; with gradients disabled it returns what ops.cosine_sim does."""
    table, rows, protos, _, _, gen = _inputs(R, D, P, fan, seed=R + D + P + fan)
    e = table[rows.long()]
    _assert_away_from_kinks(e, protos, torch.zeros(1))
    G = torch.randn(R, P, generator=gen) / R
    truth, cpu16, cpu1 = _three(lambda dt: _cos_cpu(e, protos, G, dt))
    t, p = table.to(DEV).requires_grad_(True), protos.to(DEV).requires_grad_(True)
    cos = S().ops.ProtoCosFn.apply(t, rows.to(DEV), p)
    (cos * G.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    gpu = (cos.detach().cpu(), t.grad.cpu()[rows.long()], p.grad.cpu())
    rep = Report(f'proto_cos R={R} D={D} P={P}')
    for n, what in enumerate(('cos', 'dE', 'dP')):
        rep.kappa(what, gpu[n], cpu16[n], cpu1[n], truth[n])
    rep.finish()
    with torch.no_grad():
        plain = S().ops.ProtoCosFn.apply(t, rows.to(DEV), p)
    assert not plain.requires_grad and torch.equal(plain.cpu(), gpu[0])
    rep = Report(f'proto_cos against ops.cosine_sim R={R} D={D} P={P}')
    rep.kappa('cos', S().ops.cosine_sim(t.detach(), rows.to(DEV), p.detach()).cpu(), cpu16[0], cpu1[0], truth[0])
    rep.finish()


# ---- 3. duplicate indices ---------------------------------------------------------------------------------------------------------------
def test_proto_score_duplicate_indices_at_both_table_gradients():
    """idx and widx that name rows several times (and leave some out): both scattered table gradients equal the float64 sums."""
    n_table, n_wt, R, D, P, fan = 30, 50, 200, 100, 20, 3
    table, _, protos, wt, _, gen = _inputs(n_table - 3, D, P, fan, seed=91)
    wt = wt[:n_wt]
    assert len(table) == n_table and len(wt) == n_wt
    rows = torch.randint(0, n_table - 2, (R,), generator=gen).to(torch.int32)              # the last two rows of either table are
    widx = torch.randint(0, n_wt - 2, (R * fan,), generator=gen).to(torch.int32)           # never named
    _assert_away_from_kinks(table, protos, wt)
    G = torch.randn(R, fan, generator=gen) / R

    def cpu(dtype):
        t, p, w = (x.to(dtype).clone().requires_grad_(True) for x in (table, protos, wt))
        out = protomfs_ref.score(t[rows.long()], p, w[widx.long()].reshape(R, fan, P))
        (out * G.to(dtype)).sum().backward()
        return out.detach(), t.grad, p.grad, w.grad

    truth, cpu16, cpu1 = _three(cpu)
    t, p, w = (x.to(DEV).requires_grad_(True) for x in (table, protos, wt))
    out = S().ops.ProtoScoreFn.apply(t, rows.to(DEV), p, w, widx.to(DEV), fan)
    (out * G.to(DEV)).sum().backward()
    gpu = (out.detach().cpu(), t.grad.cpu(), p.grad.cpu(), w.grad.cpu())
    assert float(gpu[1][n_table - 2:].abs().max()) == 0. and float(gpu[3][n_wt - 2:].abs().max()) == 0.
    rep = Report('proto_score with duplicate indices')
    for n, what in enumerate(('out', 'd table', 'dP', 'd weights')):
        rep.kappa(what, gpu[n], cpu16[n], cpu1[n], truth[n])
    rep.finish()


# ---- 4. kinks, compared exactly ---------------------------------------------------------------------------------------------------------
def test_proto_cos_colinear_rows_stay_in_range():
    """rows that are positive / negative multiples of a prototype: every cosine inside [-1, 1], within 1e-6 of +-1 on the diagonal"""
    gen = torch.Generator().manual_seed(3)
    for D, P in ((100, 20), (128, 64), (7, 3), (33, 65)):
        protos = torch.randn(P, D, generator=gen)
        scale = torch.logspace(-3, 3, P).unsqueeze(1)
        table = torch.cat([protos * scale, -protos * scale]).to(DEV)
        cos = S().ops.ProtoCosFn.apply(table, None, protos.to(DEV)).cpu()
        assert bool((cos >= -1).all()) and bool((cos <= 1).all())
        d = torch.arange(P)
        assert float((cos[d, d] - 1).abs().max()) <= 1e-6 and float((cos[P + d, d] + 1).abs().max()) <= 1e-6
        # the score form on the same rows: |out| <= sum_p relu(w)
        w = torch.rand(2 * P, P, generator=gen).to(DEV)
        out = S().ops.ProtoScoreFn.apply(table, torch.arange(2 * P, device=DEV), protos.to(DEV), w, None, 1)
        assert bool((out.abs().cpu() <= w.sum(dim=1, keepdim=True).cpu() * (1 + 1e-6)).all())


def test_proto_score_zero_row_takes_the_eps_clamp():
    """A zero embedding row: cos is exactly 0, out exactly 0 and finite everywhere. Its gradient is NOT zero in the reference (the G21
    case d_u_zero_row records 1e9-sized entries): F.normalize divides by max(|e|, 1e-12), so dE = sum_p dcos_p P^_p / 1e-12 with the
    projection term switched off by the clamp — finite, and compared with float64 autograd under the three-way criterion. The zero row
    contributes exactly nothing to dP (its normalised row is 0)."""
    R, D, P, fan = 70, 33, 20, 3
    table, rows, protos, wt, widx, gen = _inputs(R, D, P, fan, seed=17)
    zero = int(rows[5])
    table[zero] = 0.
    e, w = table[rows.long()], wt[widx.long()].reshape(R, fan, P)
    G = torch.randn(R, fan, generator=gen) / R
    truth, cpu16, cpu1 = _three(lambda dt: _score_cpu(e, protos, w, G, dt))
    t, p, wg = (x.to(DEV).requires_grad_(True) for x in (table, protos, wt))
    out = S().ops.ProtoScoreFn.apply(t, rows.to(DEV), p, wg, widx.to(DEV), fan)
    (out * G.to(DEV)).sum().backward()
    assert bool(torch.isfinite(out).all()) and float(out[5].abs().max()) == 0.
    assert all(bool(torch.isfinite(x.grad).all()) for x in (t, p, wg))
    assert float(wg.grad.cpu()[widx.long()].reshape(R, fan, P)[5].abs().max()) == 0.        # g cos [w > 0] with cos == 0
    gpu = (out.detach().cpu(), t.grad.cpu()[rows.long()], p.grad.cpu())
    rep = Report('proto_score with a zero row')
    for n, what in enumerate(('out', 'dE', 'dP')):
        rep.kappa(what, gpu[n], cpu16[n], cpu1[n], truth[n])
    rep.kappa('dE of the zero row', gpu[1][5], cpu16[1][5], cpu1[1][5], truth[1][5])
    rep.finish()
    # the zero row's share of every dP partial is exactly 0: the same bits as with its upstream gradient set to 0
    t2, p2 = table.to(DEV).requires_grad_(True), protos.to(DEV).requires_grad_(True)
    cos = S().ops.ProtoCosFn.apply(t2, rows.to(DEV), p2)
    Gc = torch.randn(R, P, generator=gen).to(DEV)
    (cos * Gc).sum().backward()
    assert float(cos[5].abs().max()) == 0.
    p3 = protos.to(DEV).requires_grad_(True)
    Gc0 = Gc.clone()
    Gc0[5] = 0.
    (S().ops.ProtoCosFn.apply(table.to(DEV), rows.to(DEV), p3) * Gc0).sum().backward()
    assert torch.equal(p2.grad, p3.grad)


def test_proto_score_relu_gate_is_exact():
    """w == 0 and w < 0: exactly zero gradient, and exactly no contribution to out (the same bits as with those entries set to 0)."""
    R, D, P, fan = 130, 64, 70, 3
    table, rows, protos, wt, widx, gen = _inputs(R, D, P, fan, seed=23)
    assert bool((wt == 0).any()) and bool((wt < 0).any())
    ops = S().ops
    t, p, wg = table.to(DEV), protos.to(DEV), wt.to(DEV).requires_grad_(True)
    out = ops.ProtoScoreFn.apply(t, rows.to(DEV), p, wg, widx.to(DEV), fan)
    out.sum().backward()
    assert float(wg.grad[wg.detach() <= 0].abs().max()) == 0.
    used = torch.zeros(len(wt), dtype=torch.bool)
    used[widx.long()] = True
    live = (wt > 0) & used.unsqueeze(1)
    assert bool((wg.grad.cpu()[live] != 0).any())
    gated = ops.ProtoScoreFn.apply(t, rows.to(DEV), p, wt.clamp(min=0.).to(DEV), widx.to(DEV), fan)
    assert torch.equal(out.detach(), gated)
    # the order form (widx None) is the same arithmetic
    ordered = ops.ProtoScoreFn.apply(t, rows.to(DEV), p, wt[widx.long()].to(DEV), None, fan)
    assert torch.equal(out.detach(), ordered)


def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize('R,D,P', [(3, 1, 2), (65, 33, 65), (130, 100, 70)])
def test_sim_and_cos_entries_share_one_backward(R, D, P):
    """sbr_proto_sim_* and sbr_proto_score_* (cosine form) are one front end and one backward (csrc/proto_cos.hip), compared in bits on
    rows named several times: ops.cosine_sim == ops.ProtoCosFn (the same cosine, clamped to [-1, 1]); and with a random G [R, P] into the
    similarity and nothing into ProtoSimFn's two losses (autograd materialises zeros: the arg-min terms subtract 0) the table gradient
    and dP of ProtoSimFn == those of ProtoCosFn. Every cosine is away from +-1 (asserted; D = 1: exactly +-1, which both closed intervals
    pass), so both clamps pass every element and g' is G in both. Deterministic mode fixes the order in which the table gradient adds the
    rows of a duplicate."""
    ops = S().ops
    table, _, protos, _, _, gen = _inputs(R, D, P, 1, seed=R + D + P)
    rows = torch.randint(0, R + 3, (R,), generator=gen).to(torch.int32)
    rows[-1] = rows[0]
    assert len(rows.unique()) < R
    _assert_away_from_kinks(table[rows.long()], protos, torch.zeros(1))
    G, idx = torch.randn(R, P, generator=gen).to(DEV), rows.to(DEV)
    got = {}
    prev = ops.set_deterministic(True)
    try:
        for name, fn in (('sim', lambda t, p: ops.ProtoSimFn.apply(t, idx, p)[0]), ('cos', lambda t, p: ops.ProtoCosFn.apply(t, idx, p))):
            t, p = table.to(DEV).requires_grad_(True), protos.to(DEV).requires_grad_(True)
            out = fn(t, p)
            (out * G).sum().backward()
            got[name] = (out.detach(), t.grad, p.grad)
    finally:
        ops.set_deterministic(prev)
    assert torch.equal(_bits(ops.cosine_sim(table.to(DEV), idx, protos.to(DEV))), _bits(got['cos'][0])), 'cosine_sim != ProtoCosFn'
    for n, what in ((1, 'table gradient'), (2, 'dP')):
        assert tuple(got['sim'][n].shape) == tuple(got['cos'][n].shape)
        assert torch.equal(_bits(got['sim'][n]), _bits(got['cos'][n])), f'{what} of ProtoSimFn != that of ProtoCosFn'
        assert D == 1 or bool((got['cos'][n] != 0).any()), f'{what} is all zero'


# ---- 5. the fused route against the composed one ------------------------------------------------------------------------------------
ROUTE_CONFS = [('uprotomfs', dict(embedding_dim=100, n_prototypes=20)), ('iprotomfs', dict(embedding_dim=100, n_prototypes=20)),
               ('uiprotomfs', dict(embedding_dim=48, u_n_prototypes=20, i_n_prototypes=12)),
               ('uprotomfs', dict(embedding_dim=33, n_prototypes=70))]


def _oracle_step(alg, sd_src, batch, kind, dtype):
    sd = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in sd_src.items()}
    u, i, labels = batch
    logits = protomfs_ref.forward(alg, sd, u, i)
    loss = protomfs_ref.rec_loss(kind, logits, labels)
    loss.backward()
    return {'logits': logits.detach(), 'loss': loss.detach().double().reshape(1)}, {k: v.grad for k, v in sd.items()}


@pytest.mark.parametrize('alg,conf', ROUTE_CONFS, ids=lambda v: v if isinstance(v, str) else f'{v["embedding_dim"]}')
def test_fused_forward_agrees_with_the_composed_route(alg, conf):
    """forward() (one ProtoScoreFn per prototype side) and combine(get_user_representations, get_item_representations) on the same model
    and batch (600 users x 400 items, 512 users with 1 + 3 items): logits, BCE and BPR loss and every gradient of BOTH routes against
    float64 under the three-way criterion. Unit-scale parameters, as in G21."""
    Sm = S()
    ds = Sm.SyntheticDataset(600, 400, 20000, seed=5, n_negative_samples=3, holdout_per_user=1)
    torch.manual_seed(5)
    net = Sm.ALGORITHMS[alg].build_from_conf(conf, ds)
    np.random.seed(512)
    batch = next(iter(Sm.NegativeSamplingDataLoader(ds, batch_size=512, shuffle=True)))
    gen = torch.Generator().manual_seed(6)
    sd0 = {k: torch.randn(v.shape, generator=gen) * 0.5 for k, v in net.state_dict().items()}
    net.load_state_dict(sd0)
    net.to(DEV).train()
    u, i, labels = (t.to(DEV) for t in batch)
    routes = {'fused': lambda: net(u, i),
              'composed': lambda: net.combine_user_item_representations(net.get_user_representations(u), net.get_item_representations(i))}
    rep = Report(f'{alg} {conf}: fused and composed route')
    for kind in ('bce', 'bpr'):
        truth, cpu16, cpu1 = _three(lambda dt: _oracle_step(alg, sd0, batch, kind, dt))
        for route, fn in routes.items():
            net.zero_grad()
            logits = fn()
            assert tuple(logits.shape) == tuple(i.shape)
            loss = _loss(kind, ds.n_items).compute_loss(logits, labels)
            loss.backward()
            got = {'logits': logits.detach().cpu(), 'loss': loss.detach().cpu().reshape(1)}
            for k in got:
                rep.kappa(f'{route} {kind} {k}', got[k], cpu16[0][k], cpu1[0][k], truth[0][k], f'{route} {k}')
            for k, p in net.named_parameters():
                rep.kappa(f'{route} {kind} grad {k}', p.grad.cpu(), cpu16[1][k], cpu1[1][k], truth[1][k], f'{route} grad {k}')
    rep.finish()


# ---- 6. deterministic mode ----------------------------------------------------------------------------------------------------------------
DET_CONFS = {'uprotomfs': dict(embedding_dim=100, n_prototypes=20), 'iprotomfs': dict(embedding_dim=33, n_prototypes=70),
             'uiprotomfs': dict(embedding_dim=48, u_n_prototypes=20, i_n_prototypes=12)}


def _train_steps(alg, seed, steps=12):
    Sm = S()
    Sm.reproducible(seed)
    ds = Sm.SyntheticDataset(400, 300, 9000, seed=1, n_negative_samples=3)
    net = Sm.ALGORITHMS[alg].build_from_conf(DET_CONFS[alg], ds)
    conf = {'learn': {'lr': 1e-3, 'wd': 1e-4, 'optimizer': 'adamw'}, 'run_settings': {'device': DEV}}
    tr = Sm.Trainer(net, None, None, _loss('bce', 300), conf)
    net.train()
    it = iter(Sm.NegativeSamplingDataLoader(ds, batch_size=128, shuffle=True))
    for _ in range(steps):
        tr.train_step(*next(it))
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


@pytest.mark.parametrize('alg', list(DET_CONFS))
def test_protomfs_deterministic_training_is_bit_identical(alg):
    ops = S().ops
    prev = ops.is_deterministic()
    try:
        ops.nondeterministic_launches(reset=True)
        a = _train_steps(alg, 123)
        b = _train_steps(alg, 123)
        assert ops.nondeterministic_launches() == 0
        assert ops.is_deterministic()
        for k in a:
            assert torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)), k
        assert any(not torch.equal(a[k], torch.zeros_like(a[k])) for k in a)
    finally:
        ops.set_deterministic(prev)


# ---- 7. evaluation ----------------------------------------------------------------------------------------------------------------------
class _EvalWorld:
    def __init__(self, alg, conf, n_users=1000, n_items=2000):
        Sm = S()
        self.n_users = n_users
        self.ds = Sm.SyntheticDataset(n_users, n_items, 30000, seed=4, n_negative_samples=3, holdout_per_user=1)
        torch.manual_seed(11)
        self.net = Sm.ALGORITHMS[alg].build_from_conf(conf, self.ds)
        gen = torch.Generator().manual_seed(12)
        self.net.load_state_dict({k: torch.randn(v.shape, generator=gen) * 0.5 for k, v in self.net.state_dict().items()})
        self.net.to(DEV).eval()
        self.view = self.ds.eval_view()
        sd = {k: v.detach().cpu().double() for k, v in self.net.state_dict().items()}
        with torch.no_grad():
            self.u64 = protomfs_ref.representations(alg, sd, 'user', torch.arange(n_users))
            self.i64 = protomfs_ref.representations(alg, sd, 'item', torch.arange(n_items))
            self.scores = protomfs_ref.combine(alg, self.u64, self.i64).to(DEV)
        self.excluded = torch.from_numpy(self.view.exclude_data.toarray() != 0).to(DEV)
        self.masked = self.scores.masked_fill(self.excluded, -float('inf'))

    def lists(self, scorer, top_k=(1, 10, 20)):
        Sm = S()
        ev = Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=top_k), dataset=self.view)
        got = []
        loader = type('L', (), {'dataset': self.view, 'batch_size': 512})()
        Sm.evaluation._score_split(self.net, loader, ev, DEV, scorer, None, False, 32, lambda s, u_, v, ix: got.append((v, ix)))
        return torch.cat([g[0] for g in got]), torch.cat([g[1] for g in got])


@pytest.fixture(scope='module')
def eval_world_64():
    return _EvalWorld('uprotomfs', dict(embedding_dim=100, n_prototypes=64))


@pytest.mark.parametrize('scorer', ['fp32', 'fp16_fused', 'fp32_fused'])
def test_uprotomfs_evaluation_lists_against_float64(eval_world_64, scorer):
    """uprotomfs with 64 prototypes (representations 64 wide: the fused routes take it), 1,000 users x 2,000 items, top-20 lists of every
    route against the float64 scores' ranking with the near-tie acceptance of tests/scorer_truth_util.py and the per-route bound of
    tests/test_hip_protomf.py (operands in [-1, 1] and relu'd weights: no larger than ProtoMF's); then the metrics."""
    w = eval_world_64
    L = import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')
    L.CALL_LOG = []
    try:
        got = w.lists(scorer)
        names = {n for n, _ in L.CALL_LOG}
    finally:
        L.CALL_LOG = None
    assert any(n.startswith('sbr_score_topk_f') for n in names) == (scorer != 'fp32'), names
    assert 'sbr_proto_score_fwd' in names
    mag = (w.u64.abs() @ w.i64.abs().t()).to(DEV)
    T.check_against_truth(got, torch.arange(w.n_users, device=DEV), w.masked, PM.ROUTE_C[scorer] * 2.0 ** -24 * mag, 20, what=scorer)
    metrics, _ = PM._eval(w.net, w.view, scorer)
    assert 0.0 <= metrics['ndcg@10'] <= 1.0


def test_uprotomfs_default_width_falls_back_to_fp32():
    """n_prototypes = 20: no fused scorer is built for 20-wide representations, so a fused request takes the fp32 route, exactly as for
    UProtoMF — and its metrics equal the float64 restatement's."""
    w = _EvalWorld('uprotomfs', dict(embedding_dim=100, n_prototypes=20))
    L = import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')
    ref = PM._eval(w.net, w.view, 'fp32')
    L.CALL_LOG = []
    try:
        got = PM._eval(w.net, w.view, 'fp16_fused')
        names = {n for n, _ in L.CALL_LOG}
    finally:
        L.CALL_LOG = None
    assert not any(n.startswith('sbr_score_topk_f') for n in names), names
    assert got[0] == ref[0]
    PM._same_metrics(ref, PM._metrics_from_scores(w.view, w.masked), w.n_users, 'uprotomfs 20')


# ---- 8. end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alg', list(DET_CONFS))
def test_protomfs_fit(tmp_path, alg):
    Sm = S()
    torch.manual_seed(0)
    np.random.seed(0)
    ds = Sm.SyntheticDataset(500, 300, 15000, seed=2, n_negative_samples=4, holdout_per_user=1)
    net = Sm.ALGORITHMS[alg].build_from_conf(DET_CONFS[alg], ds)
    loader = Sm.NegativeSamplingDataLoader(ds, batch_size=256, shuffle=True)
    val = type('L', (), {'dataset': ds.eval_view(), 'batch_size': 256})()
    conf = {'learn': {'lr': 1e-3, 'wd': 0., 'optimizer': 'adam', 'n_epochs': 2}, 'run_settings': {'device': DEV},
            'eval': Sm.evaluation._Cfg(top_k=(10,)), 'results_path': str(tmp_path)}
    tr = Sm.Trainer(net, loader, val, _loss('bce', 300, 4), conf)
    losses = tr.train()
    assert list(losses) == ['train/loss', 'train/rec_loss', 'train/reg_loss']
    assert all(np.isfinite(v) for v in losses.values()) and losses['train/reg_loss'] == 0
    best = tr.fit()
    pv_keys = list(STATS) if alg != 'uiprotomfs' else [f'{s}_{k}' for s in ('user', 'item') for k in STATS]
    for k in pv_keys:
        assert k in best and isinstance(best[k], float) and np.isfinite(best[k]), (k, best.get(k))
        if 'proto' in k:
            assert -1.0 <= best[k] <= 1.0, (k, best[k])
    assert np.isfinite(best['ndcg@10']) and 0.0 <= best['ndcg@10'] <= 1.0
    assert tr.train()['train/loss'] < losses['train/loss']
    # the combine class predicts the sum of its two models
    if alg == 'uiprotomfs':
        um, im = Sm.UProtoMFs(500, 300, 16, 8).to(DEV), Sm.IProtoMFs(500, 300, 16, 8).to(DEV)
        u, i = torch.arange(7, device=DEV), torch.arange(21, device=DEV).reshape(7, 3)
        with torch.no_grad():
            assert torch.equal(Sm.UIProtoMFsCombine(um, im).predict(u, i), um.predict(u, i) + im.predict(u, i))


# ---- 9. shapes outside the range, and no rows -----------------------------------------------------------------------------------------
def test_proto_score_shapes_outside_the_range_raise_and_no_rows_is_legal():
    ops = S().ops
    idx = torch.zeros(2, dtype=torch.long, device=DEV)
    for D, P in ((513, 20), (100, 1), (100, 257)):
        with pytest.raises(ValueError, match='n_prototypes'):
            ops.ProtoCosFn.apply(torch.zeros(3, D, device=DEV), None, torch.zeros(P, D, device=DEV))
        with pytest.raises(ValueError, match='n_prototypes'):
            ops.ProtoScoreFn.apply(torch.zeros(3, D, device=DEV), idx, torch.zeros(P, D, device=DEV), torch.zeros(2, P, device=DEV), None, 1)
    L = import_module(ops.__name__.rsplit('.', 1)[0] + '._lib')
    x = torch.zeros(4, 8, device=DEV)
    for n_proto, fan in ((1, 1), (257, 1), (4, 0)):                    # the entry points themselves refuse through sbr_last_error
        with pytest.raises(S().SibrarHipError, match='n_proto'):
            L.call('sbr_proto_score_fwd', x.data_ptr(), 8, None, 4, 8, x.data_ptr(), n_proto, None, 0, None, fan, x.data_ptr(), None, None,
                   None, None, x.data_ptr(), 0, L.stream())
        with pytest.raises(S().SibrarHipError, match='n_proto'):
            L.call('sbr_proto_score_bwd', x.data_ptr(), x.data_ptr(), 8, None, 4, 8, x.data_ptr(), n_proto, None, 0, None, fan, x.data_ptr(),
                   x.data_ptr(), x.data_ptr(), None, None, None, None, 0, L.stream())
    none = torch.zeros(0, dtype=torch.long, device=DEV)
    t, p = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    w = torch.zeros(0, 4, device=DEV, requires_grad=True)
    out = ops.ProtoScoreFn.apply(t, none, p, w, None, 3)
    assert tuple(out.shape) == (0, 3)
    out.sum().backward()
    assert float(p.grad.abs().max()) == 0. and float(t.grad.abs().max()) == 0. and tuple(w.grad.shape) == (0, 4)
    cos = ops.ProtoCosFn.apply(t, none, p)
    assert tuple(cos.shape) == (0, 4)
    p.grad = None
    cos.sum().backward()
    assert tuple(p.grad.shape) == (4, 8) and float(p.grad.abs().max()) == 0.
