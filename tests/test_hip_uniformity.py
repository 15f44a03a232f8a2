"""The entries of csrc/directau.hip on the GPU: 'sbr_uniformity_workspace', 'sbr_uniformity_fwd' and 'sbr_uniformity_bwd' against float64
inside the derived bound of tests/directau_ref.py (forward and gradient), duplicates and the excluded diagonal, the bits over max_wg, runs
and the deterministic mode, guard bands, refusals, the upstream gradient; 'sbr_align_fwd' and 'sbr_align_bwd' against float64."""
from importlib import import_module

import numpy as np
import pytest
import torch

import directau_ref as R
from hip_testutil import DEV, S, _Buf, _assert_bits, call, stream

pytestmark = pytest.mark.gpu


def _lib():
    return import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def ws_bytes(n, D):
    return int(_lib().lib().sbr_uniformity_workspace(n, D))


def raw(x, t, max_wg=0, g=1.0):
    """both entries on _Buf operands -> (S, loss, dx) on the host, guard bands checked"""
    n, D = x.shape
    xb = _Buf(n, D, data=t32(x))
    before = xb.flat.clone()
    out = _Buf(1, 2)
    ws = torch.empty(ws_bytes(n, D) // 8, device=DEV, dtype=torch.float64)
    call('sbr_uniformity_fwd', xb.ptr, n, D, float(t), out.ptr, out.ptr + 4, ws.data_ptr(), 8 * ws.numel(), max_wg, stream())
    sl = out.check_untouched(what='S and loss')
    gb = _Buf(1, 1, data=torch.tensor([[g]]))
    dx = _Buf(n, D)
    call('sbr_uniformity_bwd', xb.ptr, n, D, float(t), out.ptr, gb.ptr, dx.ptr, max_wg, stream())
    got = dx.check_untouched(what='dx')
    assert not bool(torch.isnan(got).any()), 'every element of dx is written'
    assert torch.equal(xb.flat.view(torch.int32), before.view(torch.int32)), 'x is read only'
    assert float(gb.host()) == g and torch.equal(out.host(), sl)
    return sl[0, 0].clone(), sl[0, 1].clone(), got.clone()


def check(x, t, what, max_wg=0):
    S_, loss, dx = raw(x, t, max_wg)
    loss64, s64 = R.uniformity64(x, t)
    e_s, e_l = abs(float(S_) - s64), abs(float(loss) - loss64)
    err = (dx.double() - torch.from_numpy(R.uniformity_grad64(x, t))).abs()
    bound = torch.from_numpy(R.grad_bound(x, t))
    print(f'{what}: S error {e_s / s64:.3e} (rel) of {R.s_rel(x, t):.3e}, loss error {e_l:.3e} of {R.loss_bound(x, t):.3e}, gradient error '
          f'{float(err.max()):.3e} of {float(bound.max()):.3e}')
    assert e_s <= R.s_rel(x, t) * s64, what
    assert e_l <= R.loss_bound(x, t), what
    assert bool((err <= bound).all()), f'{what}: {int((err > bound).sum())} gradient elements over the bound'
    return S_, loss, dx


# a sparse cross of n in {2, 3, 63, 64, 65, 128, 129, 200} and D in {1, 31, 32, 33, 64, 100, 256}: every n and every D at least twice
CROSS = [(2, 1), (2, 64), (3, 31), (3, 256), (63, 32), (63, 100), (64, 33), (64, 64), (65, 1), (65, 256), (128, 31), (128, 64), (129, 32),
         (129, 100), (200, 33), (200, 256), (200, 64)]


@pytest.mark.parametrize('n, D', CROSS)
def test_unit_rows_against_float64(n, D):
    for t in (0.5, 2.0, 16.0):
        check(R.rows(n, D, 0), t, f'n={n} D={D} t={t} unit')


@pytest.mark.parametrize('n, D', [(3, 33), (64, 31), (65, 64), (129, 256), (200, 100)])
def test_unnormalised_rows_against_float64(n, D):
    """norms up to 2: d^2 <= 16, so t in {0.5, 2} keeps t d^2 below 80 (t = 16 is inside the domain for unit rows only)"""
    for t in (0.5, 2.0):
        check(R.rows(n, D, 1, unit=False, max_norm=2.0), t, f'n={n} D={D} t={t} norms up to 2')


def test_duplicate_rows_are_ordinary_pairs():
    x = R.rows(130, 48, 2, dup=0.3)
    assert len(np.unique(x, axis=0)) <= 130 - 30
    check(x, 2.0, 'a batch with 30 % copies')


def test_two_identical_rows():
    x = np.tile(R.rows(1, 24, 3), (2, 1))
    S_, loss, dx = check(x, 2.0, 'two identical rows')
    assert abs(float(S_) - 1.0) <= R.s_rel(x, 2.0)
    assert bool((dx.double().abs() <= torch.from_numpy(R.grad_bound(x, 2.0))).all())


@pytest.mark.parametrize('t', [0.5, 2.0, 16.0])
def test_the_diagonal_is_excluded(t):
    """two orthogonal unit rows: one pair of d^2 = 2, so loss = -2 t; a counted diagonal would add two terms of weight 1"""
    x = np.eye(2, 40, dtype=np.float32)
    _, loss, _ = check(x, t, f'orthogonal pair t={t}')
    assert abs(float(loss) + 2 * t) <= R.loss_bound(x, t)


def test_bits_over_max_wg_runs_and_modes():
    ops = S().ops
    x = R.rows(200, 40, 5, dup=0.1)
    base = raw(x, 2.0, 0)
    for max_wg in (1, 2, 0):
        for a, b, name in zip(base, raw(x, 2.0, max_wg), ('S', 'loss', 'dx')):
            _assert_bits(b.reshape(-1), a.reshape(-1), f'{name} at max_wg={max_wg}')
    prev = ops.set_deterministic(True)
    try:
        ops.nondeterministic_launches(reset=True)
        for max_wg in (0, 1):
            for a, b, name in zip(base, raw(x, 2.0, max_wg), ('S', 'loss', 'dx')):
                _assert_bits(b.reshape(-1), a.reshape(-1), f'{name} in deterministic mode at max_wg={max_wg}')
        xd = t32(x).to(DEV).requires_grad_()
        ops.UniformityFn.apply(xd, 2.0).backward()
        _assert_bits(xd.grad.cpu(), base[2], 'UniformityFn in deterministic mode')
        lab = torch.zeros(37, 4, dtype=torch.float64)
        lab[:, 0] = 1
        ops.AlignLossFn.apply(torch.randn(37, 4, device=DEV, requires_grad=True), lab, 1 / 37).backward()
        assert ops.nondeterministic_launches() == 0
    finally:
        ops.set_deterministic(prev)
    assert ops.nondeterministic_launches() == 0


def test_refusals_launch_nothing():
    L = _lib()
    x = _Buf(8, 16, data=t32(R.rows(8, 16, 6)))
    out, g, dx = _Buf(1, 2), _Buf(1, 1, fill=1.0), _Buf(8, 16)
    ws = torch.empty(1, device=DEV, dtype=torch.float64)
    fwd = lambda **k: ('sbr_uniformity_fwd', [k.get('x', x.ptr), k.get('n', 8), k.get('D', 16), k.get('t', 2.0), k.get('S', out.ptr),       # noqa: E731
                                              k.get('loss', out.ptr + 4), k.get('ws', ws.data_ptr()), k.get('wsb', 8), k.get('wg', 0), stream()])
    bwd = lambda **k: ('sbr_uniformity_bwd', [k.get('x', x.ptr), k.get('n', 8), k.get('D', 16), k.get('t', 2.0), k.get('S', out.ptr),       # noqa: E731
                                              k.get('g', g.ptr), k.get('dx', dx.ptr), k.get('wg', 0), stream()])
    cases = [fwd(n=1), fwd(n=0), fwd(D=0), fwd(D=257), fwd(t=0.0), fwd(t=-2.0), fwd(t=float('inf')), fwd(x=None), fwd(S=None), fwd(loss=None),
             fwd(ws=None), fwd(wsb=7), fwd(n=65, wsb=8), fwd(wg=-1),
             bwd(n=1), bwd(D=0), bwd(D=257), bwd(t=0.0), bwd(x=None), bwd(S=None), bwd(g=None), bwd(dx=None), bwd(dx=x.ptr),
             bwd(dx=x.ptr + 4 * 16), bwd(wg=-1),
             ('sbr_align_fwd', [None, g.ptr, 1, 1, 1.0, g.ptr, stream()]), ('sbr_align_fwd', [x.ptr, g.ptr, -1, 1, 1.0, g.ptr, stream()]),
             ('sbr_align_fwd', [x.ptr, g.ptr, 1, 0, 1.0, g.ptr, stream()]), ('sbr_align_bwd', [None, 1, 1, 1.0, g.ptr, 0, dx.ptr, stream()]),
             ('sbr_align_bwd', [g.ptr, 1, 1, 1.0, None, 0, dx.ptr, stream()]), ('sbr_align_bwd', [g.ptr, 1, 0, 1.0, g.ptr, 0, dx.ptr, stream()])]
    for name, args in cases:
        with pytest.raises(S().SibrarHipError, match=name):
            call(name, *args)
    out.check_untouched(written_rows=[], what='S and loss after refused calls')
    dx.check_untouched(written_rows=[], what='dx after refused calls')
    assert ws_bytes(200, 64) == 8 * 4 and ws_bytes(64, 1) == 8 and ws_bytes(65, 256) == 16
    with pytest.raises(S().SibrarHipError, match='sbr_uniformity_fwd'):
        S().ops.uniformity(torch.randn(1, 8, device=DEV))
    with pytest.raises(S().SibrarHipError, match='sbr_uniformity_fwd'):
        S().ops.uniformity(torch.randn(4, 257, device=DEV))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S().ops.uniformity(torch.randn(4, 8))


def test_the_upstream_gradient_is_honoured():
    """4 x: every product by a power of two is exact, the same bits scaled. 3 x: coef = fl(3 c) and one product each way differ by at most
    three roundings: |dx3 - 3 dx1| <= 1.01 * 3 u |3 dx1|. ops.uniformity agrees with the raw entries bit for bit."""
    ops = S().ops
    x = R.rows(129, 20, 7)
    S_, loss, dx = raw(x, 2.0)
    got_loss, got_S = ops.uniformity(t32(x).to(DEV), 2.0, max_wg=1)
    _assert_bits(got_loss.cpu().reshape(1), loss.reshape(1), 'ops.uniformity: loss')
    _assert_bits(got_S.cpu().reshape(1), S_.reshape(1), 'ops.uniformity: S')
    grads = {}
    for k in (1.0, 3.0, 4.0):
        xd = t32(x).to(DEV).requires_grad_()
        out = ops.UniformityFn.apply(xd, 2.0)
        _assert_bits(out.detach().cpu().reshape(1), loss.reshape(1), 'UniformityFn: loss')
        (k * out).backward()
        grads[k] = xd.grad.cpu()
    _assert_bits(grads[1.0], dx, 'UniformityFn: gradient')
    _assert_bits(grads[4.0], 4 * dx, 'four times the loss')
    assert bool(((grads[3.0].double() - 3 * dx.double()).abs() <= 1.01 * 3 * R.U * (3 * dx.double()).abs()).all())
    assert float(grads[3.0].abs().max()) > 0


@pytest.mark.parametrize('aggregator', ['mean', 'sum'])
@pytest.mark.parametrize('N', [1, 5])
@pytest.mark.parametrize('B', [1, 37, 300])
def test_align_against_float64(B, N, aggregator):
    rng = np.random.default_rng(10 * B + N)
    z = rng.uniform(-1, 1, size=(B, N)).astype(np.float32)
    lab = np.zeros((B, N))
    lab[:, 0] = 1
    if N > 1 and B > 1:
        lab[B // 2, 3] = 1                                                     # once, two positives in a row
    n_pos = int(lab.sum())
    scale = 1.0 / n_pos if aggregator == 'mean' else 1.0
    zb, db = _Buf(B, N, data=t32(z)), _Buf(B, N)
    labels = torch.from_numpy(lab).to(DEV)
    out = torch.full((3,), float('nan'), device=DEV, dtype=torch.float64)
    g = torch.tensor([0.75], device=DEV, dtype=torch.float64)
    runs = []
    for _ in range(2):
        call('sbr_align_fwd', zb.ptr, labels.data_ptr(), B, N, scale, out[1:].data_ptr(), stream())
        call('sbr_align_bwd', labels.data_ptr(), B, N, scale, g.data_ptr(), 1, db.ptr, stream())
        runs.append((out.cpu().clone(), db.check_untouched(what='dlogits').clone()))
    assert bool(torch.isnan(runs[0][0][[0, 2]]).all()), 'only the scalar is written'
    want = R.align64(z, lab, scale)
    assert abs(float(runs[0][0][1]) - want) <= 1e-6 * abs(want)
    want_d = torch.from_numpy(np.where(lab == 1, np.float32(-2.0 * scale * 0.75), np.float32(0))).float()
    _assert_bits(runs[0][1], want_d, 'the gradient is -2 scale g at the positives and 0 elsewhere')
    assert torch.equal(runs[0][0][1:2], runs[1][0][1:2])
    _assert_bits(runs[0][1], runs[1][1], 'two runs')
    # the loss class: the same value, the fp32 upstream gradient of autograd
    zd = t32(z).to(DEV).requires_grad_()
    loss = S().RecAlignmentLoss(n_items=40, aggregator=aggregator, neg_train=max(N - 1, 1)).compute_loss(zd, labels)
    assert loss.dtype == torch.float64 and abs(float(loss.detach()) - want) <= 1e-6 * abs(want)
    loss.backward()
    assert bool(((zd.grad.cpu().double() - torch.from_numpy(np.where(lab == 1, -2.0 * scale, 0.0))).abs() <= 2 * R.U * 2 * scale).all())
