"""GPU: the deterministic mode (``ops.set_deterministic``; reference call site utilities/utils.py:22-27).

  1. bit identity: two trainings from the same parameters, batches, modality draws and dropout seeds — c1 (300 steps; dense and
     deferred row-wise AdamW; hipGraph on and off) and c2 at the bench shape (B = 8192 x 50 steps, B = 256 x 200 steps) — leave
     every state_dict tensor, both Adam moment buffers and every step's loss triple equal under ``torch.equal``;
  2. the counter ``sbr_nondeterministic_launches()`` stays 0 across those trainings (agreement at a small shape can be luck; the
     counter cannot) and reads > 0 for the same c1 step in default mode;
  3. default mode calls the entry-point sequence recorded on the commit before the mode existed (tests/golden);
  4. accuracy: criteria a) and c) of tests/test_hip_c1.py re-run with the mode on, that file's KAPPA and floors unchanged;
  5. kernel level: the segmented row accumulation and the fixed-slot column sum against float64 with the bounds
     tests/test_hip_rowops.py uses for the atomic forms, and two calls equal bit for bit;
  6. loud, not wrong: a path without a fixed-order form raises an error that names the entry point.
"""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import test_hip_c1 as C1T
from test_hip_c1 import c1, gpu_batch, gpu_fused                       # noqa: F401  (c1: the module-scoped fixture)
from test_hip_rowops import U32, _Buf, _assert_bound, _bits, _i32, _p, _rand

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'c1_default_call_sequence.json')


def S():
    import sibrar_amd
    return sibrar_amd


def _L():
    return importlib.import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')


@pytest.fixture
def det():
    """The mode on for one test, the counter reset; off again afterwards whatever happens."""
    ops = S().ops
    prev = ops.set_deterministic(True)
    ops.nondeterministic_launches(reset=True)
    try:
        yield ops
    finally:
        ops.set_deterministic(prev)


# ---- 5. kernel level ------------------------------------------------------------------------------------------------------------
def _scatter_patterns(n, n_table, seed):
    rng = np.random.default_rng(seed)
    return {'all_to_one': np.full(n, 7 % n_table), 'one_to_one': rng.permutation(n_table)[:n] if n <= n_table else None,
            'heavy': rng.integers(0, 53, size=n)}


@pytest.mark.parametrize('D', [64, 128, 100, 260])
@pytest.mark.parametrize('pattern,n', [('all_to_one', 3000), ('one_to_one', 1500), ('heavy', 4099), ('sentinel', 6000)])
def test_segmented_scatter_against_float64(det, D, pattern, n):
    """dW[rows[j], :] += dOut[ii(j), :] in its fixed-order form, through ``sbr_scatter_add_rows`` with the mode on and through
    ``sbr_scatter_add_rows_det``: per element |err| <= m u sum|terms| (m sources of that table row: the bound of the atomic form in
    tests/test_hip_rowops.py), unnamed rows stay +0, strided operands are not overrun, and two calls give the same bits. 'sentinel':
    770 slots name one table row through ONE zero gradient row (the padded slot lists of a captured step) among ordinary rows."""
    n_table = 2000
    rng = np.random.default_rng(n + D)
    if pattern == 'sentinel':
        rows = rng.integers(0, n_table, size=n)
        n_src = n + 1
        ii = rng.permutation(n)
        pads = rng.choice(n, size=770, replace=False)
        ii[pads] = n                                               # the zero row
        rows[pads] = rows[0]
        use_ii = True
    else:
        rows = _scatter_patterns(n, n_table, n * 7 + D)[pattern]
        n_src, use_ii = n + 5, True
        ii = rng.permutation(n_src)[:n]
    g = _rand(n_src, D, seed=n % 1000 + D)
    if pattern == 'sentinel':
        g[n] = 0.0
    else:
        kind = rng.integers(0, 12, size=n_src)
        g[kind == 0] = 0.0
        g[kind == 1] = -0.0
    src = g[torch.as_tensor(ii)]
    rt = torch.as_tensor(rows, dtype=torch.int64)
    ref = torch.zeros(n_table, D, dtype=torch.float64).index_add_(0, rt, src.double())
    mag = torch.zeros(n_table, D, dtype=torch.float64).index_add_(0, rt, src.double().abs())
    m = torch.bincount(rt, minlength=n_table).double()[:, None]
    outs = []
    for entry in ('sbr_scatter_add_rows', 'sbr_scatter_add_rows', 'sbr_scatter_add_rows_det'):
        dOut = _Buf(n_src, D, D + 4, 1, data=g)
        dW = _Buf(n_table, D, D + 8, 1, fill=0.0)
        ii_d, rows_d = _i32(ii), _i32(rows)                        # kept alive until the launches have run
        _L().call(entry, dOut.ptr, dOut.ld, _p(ii_d), _p(rows_d), dW.ptr, dW.ld, n, D, _L().stream())
        torch.cuda.synchronize()
        got = dW.check_untouched(None, entry)
        _assert_bound(got, ref, m * U32 * mag, f'{entry} {pattern} n={n} D={D}')
        assert bool((_bits(got[m[:, 0] == 0]) == 0).all()), 'a table row that no source names was written'
        outs.append(got.clone())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), 'two calls of the fixed-order form differ'
    assert det.nondeterministic_launches() == 0


@pytest.mark.parametrize('n,C', [(90_112, 128), (5632, 64), (1777, 100), (3, 260)])
def test_fixed_slot_colsum_and_batchnorm_against_float64(det, n, C):
    """``sbr_colsum`` and the BatchNorm statistics in their fixed-slot form: the column sum within n u sum|x| of float64 (looser than
    needed: the blocks add in double), batch mean / rstd through ``BatchNormActFn`` against float64, two calls equal bit for bit."""
    ops = det
    x = _rand(n, C, seed=n + C).to(DEV)
    ref = x.double().cpu().sum(0)
    a, b = ops.colsum(x).cpu(), ops.colsum(x).cpu()
    assert torch.equal(a, b)
    _assert_bound(a, ref, n * U32 * x.double().cpu().abs().sum(0) + 1e-30, f'colsum n={n} C={C}')
    w, bias = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    ys = []
    for _ in range(2):
        rm, rv, nbt = torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros(1, device=DEV, dtype=torch.int64)
        xx = x.clone().requires_grad_(True)
        y = ops.BatchNormActFn.apply(xx, w.clone().requires_grad_(True), bias.clone().requires_grad_(True), rm, rv, nbt, 0)
        y.square().sum().backward()
        ys.append((y.detach().cpu(), xx.grad.cpu(), rm.cpu(), rv.cpu()))
    for p, q in zip(*ys):
        assert torch.equal(p, q)
    xd = x.double().cpu()
    if n > 1:
        want = (xd - xd.mean(0)) / torch.sqrt(xd.var(0, unbiased=False) + ops.BN_EPS)
        assert float((ys[0][0].double() - want).abs().max()) <= 2e-5
    assert ops.nondeterministic_launches() == 0


# ---- 1. + 2. bit identity and the counter ---------------------------------------------------------------------------------------
def _train(make, batches, n_steps):
    net, opt, fused = make()
    losses = []
    for s in range(n_steps):
        losses.append(torch.stack(list(fused.step(*batches[s % len(batches)]))).clone())
    fused.close()
    torch.cuda.synchronize()
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    return state, opt.m.detach().clone(), opt.v.detach().clone(), torch.stack(losses), fused


def _assert_same(a, b, what):
    sa, ma, va, la, _ = a
    sb, mb, vb, lb, _ = b
    assert torch.isfinite(la).all(), f'{what}: a loss is not finite'
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not bad, f'{what}: state_dict tensors differ between two identical trainings: {bad}'
    assert torch.equal(ma, mb) and torch.equal(va, vb), f'{what}: Adam moments differ'
    assert torch.equal(la, lb), f'{what}: loss triples differ (first at step {int((la != lb).any(1).nonzero()[0])})'


@pytest.mark.parametrize('graph', ['0', '1'])
@pytest.mark.parametrize('deferred', ['0', '1'])
def test_c1_training_is_bit_identical(c1, det, deferred, graph, monkeypatch):
    """300 steps on the c1 fixture's recorded batches (cycled), twice from sd0 with a fresh FusedOptimizer + FusedTrainStep."""
    monkeypatch.setenv('SBR_DEFERRED_ADAM', deferred)
    monkeypatch.setenv('SBR_GRAPH', graph)
    w = c1
    batches = [gpu_batch(w, b) for b in w.batches]
    runs = [_train(lambda: gpu_fused(w, w.sd0), batches, 300) for _ in range(2)]
    assert (runs[0][4].deferred is not None) == (deferred == '1')
    if graph == '1':
        assert runs[0][4].n_replays > 200, f'only {runs[0][4].n_replays} of 300 steps were graph replays'
    else:
        assert runs[0][4].n_replays == 0
    _assert_same(runs[0], runs[1], f'c1 deferred={deferred} graph={graph}')
    n = det.nondeterministic_launches()
    assert n == 0, f'{n} launches of arrival-order float accumulation during a deterministic c1 training'


def test_counter_is_wired_and_default_mode_calls_what_it_called_before(c1):
    """The same c1 step in DEFAULT mode: the counter must read > 0 (otherwise it is not wired and the zero above proves nothing),
    and the entry points called are exactly those recorded on the commit before the mode existed (tests/golden), the GEMMs those
    of ``test_hip_c1.GEMMS``."""
    ops = S().ops
    assert not ops.is_deterministic()
    w = c1
    ops.nondeterministic_launches(reset=True)
    net, opt, fused = gpu_fused(w, w.sd0)
    lib = _L()
    lib.CALL_LOG = []
    try:
        fused.step(*gpu_batch(w, w.batches[0]))
    finally:
        log, lib.CALL_LOG = lib.CALL_LOG, None
    fused.close()
    n = ops.nondeterministic_launches()
    assert n > 0, 'the counter of arrival-order launches is not wired: a default-mode c1 step read 0'
    names = [n_ for n_, _ in log]
    assert [n_ for n_ in names if n_.startswith('sbr_gemm')] == C1T.GEMMS[256]
    want = json.load(open(GOLDEN))['c1_b256_first_step']
    assert names == want, f'default mode calls a different entry-point sequence:\n{names}\n!=\n{want}'


@pytest.fixture(scope='module')
def c2():
    bench = importlib.import_module('bench')
    ds, net = bench.build(S(), dict(bench.C2), DEV)
    net.train()
    sd0 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    lossf = S().RecSampledSoftmaxLoss(n_items=ds.n_items, aggregator='mean', train_neg_strategy='uniform_recbole',
                                      neg_train=ds.n_negative_samples)
    return ds, net, sd0, lossf


@pytest.mark.parametrize('graph', [True, False])
@pytest.mark.parametrize('B,steps', [(8192, 50), (256, 200)])
def test_c2_training_is_bit_identical(c2, det, B, steps, graph):
    """The headline bench config at its own shape (100k users x 50k items), built the way
    test_hip_pinned.test_c2_step_at_the_bench_batch_against_the_cpu_oracle builds it: 8 loader batches with recorded modality draws,
    cycled; two trainings from the same parameters."""
    ds, net, sd0, lossf = c2
    np.random.seed(42)
    loader = S().NegativeSamplingDataLoader(ds, batch_size=B, shuffle=True)
    it = iter(loader)
    raw = [next(it) for _ in range(8)]
    assert tuple(raw[0][1].shape) == (B, 11)
    made = []

    def make():
        net.load_state_dict({k: v.to(DEV) for k, v in sd0.items()})
        net.train()
        opt = S().FusedOptimizer(net, 'adamw', lr=1e-3, weight_decay=0.)
        fused = S().FusedTrainStep(net, lossf, opt, use_graph=graph)
        made.append(fused)
        return net, opt, fused

    probe = make()[2]
    batches = [(u, i, l, probe.draw(u.shape, i.shape)) for u, i, l in raw]          # one recorded draw per batch, shared by both runs
    probe.close()
    runs = [_train(make, batches, steps) for _ in range(2)]
    assert runs[0][4].deferred is not None
    if graph:
        assert runs[0][4].n_replays >= steps // 2, f'only {runs[0][4].n_replays} of {steps} steps were graph replays'
    _assert_same(runs[0], runs[1], f'c2 B={B} graph={graph}')
    n = det.nondeterministic_launches()
    assert n == 0, f'{n} launches of arrival-order float accumulation during a deterministic c2 training'


# ---- 4. accuracy is not traded away ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [256, 4096])
def test_c1_step_against_float64_in_deterministic_mode(c1, det, B):
    """Criterion a) of tests/test_hip_c1.py (one step at B = 256 and 4096 against the float64 oracle and both fp32 runs), with the
    mode on: that test's own code, KAPPA = 3.0 and floors, unchanged — a fixed-order fp32 sum is held to what an atomic one is."""
    assert C1T.KAPPA == 3.0
    C1T.test_c1_step_at_full_shape_against_float64(c1, B)
    assert det.nondeterministic_launches() == 0


@pytest.mark.parametrize('deferred', ['0', '1'])
def test_c1_trajectory_against_float64_in_deterministic_mode(c1, det, deferred, monkeypatch):
    """Criterion c) of tests/test_hip_c1.py (the 30-step trajectory, dense and deferred row-wise AdamW) with the mode on."""
    C1T.test_c1_30_step_trajectory_against_float64(c1, deferred, monkeypatch)
    assert det.nondeterministic_launches() == 0


# ---- 6. loud, not wrong ------------------------------------------------------------------------------------------------------------
def test_paths_without_a_fixed_order_form_raise(c1, det):
    """With the mode on, the scatter form of the tag-bag gradient (forced here; the step takes the gather form on its own), the
    atomic split-K of ``sbr_gemm_f32`` and the bias gradients of ``SGDBaseline`` raise an error naming the entry point instead of
    running their atomics."""
    Err = S().SibrarHipError
    w = c1
    FE = S().FeatureEmbedding
    prev = FE.CSR_GATHER_FORCE
    FE.CSR_GATHER_FORCE = False
    try:
        net, opt, fused = gpu_fused(w, w.sd0)
        with pytest.raises(Err, match=r'sbr_bag_mean_bwd: no deterministic form'):
            fused.step(*gpu_batch(w, w.batches[0]))
        fused._graphs.clear()
    finally:
        FE.CSR_GATHER_FORCE = prev
        torch.cuda.synchronize()
    a, b, c = torch.randn(64, 32, device=DEV), torch.randn(64, 16, device=DEV), torch.zeros(32, 16, device=DEV)
    with pytest.raises(Err, match=r'sbr_gemm_f32: no deterministic form'):
        det.gemm(2, a, 32, None, b, 16, None, None, c, 16, None, 32, 16, 64, 0, 1)
    g = torch.randn(8, 4, device=DEV)
    with pytest.raises(Err, match=r'sbr_bias_score_bwd: no deterministic form'):
        _L().call('sbr_bias_score_bwd', g.data_ptr(), None, None, torch.zeros(8, device=DEV).data_ptr(), None, None, 8, 4, _L().stream())
    assert det.nondeterministic_launches() == 0
