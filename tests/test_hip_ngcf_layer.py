"""NGCF's layer kernels on the GPU: 'sbr_ngcf_layer_fwd' (csrc/ngcf.hip) against its fp32 restatement bit for bit and against float64
inside the derived bound (tests/ngcf_ref.py), zero rows, an exact world, determinism over runs and row splits, 'sbr_ngcf_layer_bwd'
against float64 autograd, and the refusals.

Bit equality with the restatement is asked on EVERY input (lightgcn_ref.fma32 has no double rounding)."""
from importlib import import_module

import numpy as np
import pytest
import torch

import lightgcn_ref as L
import ngcf_ref as R
from hip_testutil import DEV, S, _Buf, _assert_bits, _assert_bound, call, stream

pytestmark = pytest.mark.gpu
FWD, BWD = 'sbr_ngcf_layer_fwd', 'sbr_ngcf_layer_bwd'
WIDE, OFF = 7, 3                                                             # the wider table has 7 more columns, the slice starts at column 3


def _mod(name):
    return import_module(S().ops.__name__.rsplit('.', 1)[0] + '.' + name)


_CSR = {}


def dev_csr(g):
    if id(g) not in _CSR:
        _CSR[id(g)] = (g, _mod('features').DeviceCSR(g.m).to(DEV))
    return _CSR[id(g)][1]


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def graph_args(g):
    csr = dev_csr(g)
    ti, tx, _ = csr.transposed()
    return [csr.indptr.data_ptr(), csr.indices.data_ptr(), ti.data_ptr(), tx.data_ptr(), g.n_users, g.n_items]


def raw_fwd(g, x, W1, W2, bias, h, out, din, dout, slope=R.SLOPE, p=0.0, seed=R.SEED, sid=R.STREAM, rows=None, ld=None, out_ptr=None):
    """the entry itself on _Buf operands; ``out`` is the wider table, the slice starts OFF columns in"""
    r0, r1 = (0, g.n) if rows is None else rows
    call(FWD, *graph_args(g), r0, r1, x.ptr, din, W1.ptr, W2.ptr, bias.ptr, dout, float(slope), float(p), seed, sid, h.ptr,
         out.ptr + 4 * OFF if out_ptr is None else out_ptr, out.ld if ld is None else ld, stream())


# ---- 1. general worlds: the restatement bit for bit, float64 inside the bound ------------------------------------------------------------
@pytest.mark.parametrize('p', R.RATES)
@pytest.mark.parametrize('width', R.WIDTHS, ids=lambda w: f'{w[0]}x{w[1]}')
@pytest.mark.parametrize('n_items', R.ITEMS)
@pytest.mark.parametrize('n_users', R.USERS)
def test_forward_against_restatement_and_float64(n_users, n_items, width, p):
    din, dout = width
    c = R.case(n_users, n_items, din, dout, p)
    g, ops = c['g'], S().ops
    what = f'{n_users} x {n_items}, {din} -> {dout}, p = {p}'
    x, W1, W2, bias = (t32(c[k]).to(DEV) for k in ('x', 'W1', 'W2', 'bias'))
    table = torch.full((g.n, dout + WIDE), 7.25, device=DEV)
    h, out = ops.ngcf_layer(dev_csr(g), x, W1, W2, bias, R.SLOPE, p, R.SEED, R.STREAM, out=table[:, OFF:OFF + dout])
    torch.cuda.synchronize()
    _assert_bits(h.cpu(), t32(c['r32']['h']), what + ': h against the restatement')
    _assert_bits(out.cpu(), t32(c['r32']['out']), what + ': out against the restatement')
    host = table.cpu()
    assert bool((host[:, :OFF] == 7.25).all()) and bool((host[:, OFF + dout:] == 7.25).all()), what + ': columns outside the slice were written'
    _assert_bound(h.cpu(), torch.from_numpy(c['r64']['h']), torch.from_numpy(c['bound']['h']), what + ': h against float64')
    _assert_bound(out.cpu(), torch.from_numpy(c['r64']['out']), torch.from_numpy(c['bound']['out']), what + ': out against float64')
    ratio = float((np.abs(out.cpu().numpy().astype(np.float64) - c['r64']['out']) / np.maximum(c['bound']['out'], 1e-300)).max())
    print(f'{what}: largest error / bound of out {ratio:.3f}')
    assert torch.equal(x.cpu(), t32(c['x'])), what + ': x changed'
    # every table one float off the 16-byte boundary (the single-float gather also where Din % 4 == 0), inside NaN guards
    bx, bw1, bw2, bb = (_Buf(*t.shape, off=1, data=t) if t.dim() == 2 else _Buf(1, t.shape[0], off=1, data=t[None])
                        for t in (t32(c['x']), t32(c['W1']), t32(c['W2']), t32(c['bias'])))
    bh, bo = _Buf(g.n, dout, off=1), _Buf(g.n, dout + WIDE, off=1, fill=7.25)
    raw_fwd(g, bx, bw1, bw2, bb, bh, bo, din, dout, p=p)
    _assert_bits(bh.check_untouched(what=what + ': h off the boundary'), t32(c['r32']['h']), what + ': h off the boundary')
    wide = bo.check_untouched(what=what + ': out off the boundary')
    _assert_bits(wide[:, OFF:OFF + dout], t32(c['r32']['out']), what + ': out off the boundary')
    assert bool((wide[:, :OFF] == 7.25).all()) and bool((wide[:, OFF + dout:] == 7.25).all())
    assert torch.equal(bx.check_untouched(), t32(c['x']))


# ---- 2. rows of zeros --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('width', [(5, 3), (64, 64), (65, 128)], ids=lambda w: f'{w[0]}x{w[1]}')
def test_all_dropped_and_empty_rows_give_plus_zero(width):
    """An all-dropped row: p = 1 - 2^-24, which only a uniform of exactly that value reaches (these seeds draw none). A row without neighbours has s = +0, so z = x W1 + bias: it
    is a row of zeros where its input row and the bias are zero (with a negative weight in every column: the products are -0, and
    +0 + -0 = +0). Both give h = +0 and out = +0 / 1e-12 = +0: no NaN, no sign bit."""
    din, dout = width
    g = R.world(257, 130)
    empty = np.flatnonzero(g.deg == 0)
    assert len(empty) >= 2
    ops = S().ops
    x = L.table(g.n, din, 11)
    x[empty] = 0
    W1, W2, _ = R.weights(din, dout)
    W1[0] = -np.abs(W1[0])
    zero = torch.zeros(dout, device=DEV)
    h, out = ops.ngcf_layer(dev_csr(g), t32(x).to(DEV), t32(W1).to(DEV), t32(W2).to(DEV), zero, R.SLOPE, 0.0)
    for t in (h, out):
        assert not bool(t[empty].any()) and not bool(torch.signbit(t[empty]).any()) and not bool(torch.isnan(t).any())
    assert bool(h[g.deg > 0].any())
    p = float(np.nextafter(np.float32(1), np.float32(0)))                        # the largest fp32 below 1: u <= 1 - 2^-24 < p
    h, out = ops.ngcf_layer(dev_csr(g), t32(x).to(DEV), t32(W1).to(DEV), t32(W2).to(DEV), t32(R.weights(din, dout)[2]).to(DEV), R.SLOPE, p, 1, 2)
    for t in (h, out):
        assert not bool(t.any()) and not bool(torch.signbit(t).any()) and not bool(torch.isnan(t).any())


# ---- 3. an exact world: float64 bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('width', [(4, 4), (5, 3), (64, 65)], ids=lambda w: f'{w[0]}x{w[1]}')
@pytest.mark.parametrize('with_empty', [False, True])
def test_exact_world_equals_float64(with_empty, width):
    """Degrees 1, 4, 16, tables in [-8, 8], weights in [-2, 2], slope 1/4: s is a multiple of 1/16 of at most 2^7, a and b multiples of
    1/16 of at most 2^8 and 2^10, every partial sum of z (at most 130 terms of at most 2^11) a multiple of 1/16 below 2^19, and slope * z
    a multiple of 1/64 below 2^17: all exact in fp32, whatever the order. h = z or z / 4, so h equal to float64 says the same of z."""
    din, dout = width
    g = L.exact_world(1, with_empty)
    rng = np.random.default_rng(3)
    x = L.int_table(g.n, din, 7)
    W1, W2 = (rng.integers(-2, 3, size=(din, dout)).astype(np.float32) for _ in range(2))
    bias = rng.integers(-4, 5, size=dout).astype(np.float32)
    ref = R.layer64(g, x, W1, W2, bias, 0.25)
    h, out = S().ops.ngcf_layer(dev_csr(g), *(t32(t).to(DEV) for t in (x, W1, W2, bias)), 0.25, 0.0)
    assert torch.equal(h.cpu().double(), torch.from_numpy(ref['h'])), 'h = LeakyReLU(z): z and h equal float64'
    assert bool((ref['h'] == ref['z'])[ref['z'] > 0].all()) and bool((ref['z'] > 0).any()) and bool((ref['z'] < 0).any())
    _assert_bits(out.cpu(), t32(R.layer32(g, x, W1, W2, bias, 0.25)['out']), 'out against the restatement')


# ---- 4. determinism: runs, splits, rows outside the range ----------------------------------------------------------------------------------
@pytest.mark.parametrize('width', [(3, 5), (64, 64), (65, 33), (128, 128)], ids=lambda w: f'{w[0]}x{w[1]}')
def test_runs_and_row_splits_give_the_same_bits(width):
    din, dout = width
    c = R.case(257, 130, din, dout, 0.3)
    g, ops = c['g'], S().ops
    nu, n = g.n_users, g.n
    x, W1, W2, bias = (t32(c[k]).to(DEV) for k in ('x', 'W1', 'W2', 'bias'))
    args = (dev_csr(g), x, W1, W2, bias, R.SLOPE, 0.3, R.SEED, R.STREAM)
    h, out = ops.ngcf_layer(*args)
    h2, out2 = ops.ngcf_layer(*args)
    _assert_bits(h2.cpu(), h.cpu(), 'second run: h')
    _assert_bits(out2.cpu(), out.cpu(), 'second run: out')
    for cuts in ([0, nu, n], [0, 1, 100, nu - 3, nu + 7, n - 1, n], [0, 0, 63, 64, 65, n]):
        hc, oc = torch.full((n, dout), 7.25, device=DEV), torch.full((n, dout), -3.5, device=DEV)
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            before_h, before_o = hc.clone(), oc.clone()
            ops.ngcf_layer(*args, h=hc, out=oc, rows=(r0, r1))
            keep = torch.ones(n, dtype=torch.bool, device=DEV)
            keep[r0:r1] = False
            assert torch.equal(hc[keep], before_h[keep]) and torch.equal(oc[keep], before_o[keep]), f'rows outside [{r0}, {r1}) were written'
        _assert_bits(hc.cpu(), h.cpu(), f'split {cuts}: h (mask included)')
        _assert_bits(oc.cpu(), out.cpu(), f'split {cuts}: out')
    ph, po = ops.ngcf_layer(*args, rows=(nu - 2, nu + 2))                                  # new results: zeros outside the range
    assert torch.equal(ph[nu - 2:nu + 2], h[nu - 2:nu + 2]) and not bool(ph[:nu - 2].any()) and not bool(po[nu + 2:].any())


# ---- 5. backward against float64 autograd --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', R.RATES)
@pytest.mark.parametrize('middle', [False, True], ids=['single', 'middle'])
@pytest.mark.parametrize('width', [(8, 8), (64, 64), (65, 33), (128, 128)], ids=lambda w: f'{w[0]}x{w[1]}')
def test_backward_against_float64_autograd(width, middle, p):
    """Tolerance: lightgcn_ref.FACTOR (8) x the error of the same formula in torch float32 on the CPU against float64 on these inputs,
    per quantity, no floor. ``middle``: the gradient of h (what the next layer sends back) is given as well as that of out. Both
    figures are printed; DESIGN.md 4.37 records the measured pairs."""
    din, dout = width
    g = R.world(257, 130)
    ops = S().ops
    x = L.table(g.n, din, 3)
    W1, W2, bias = R.weights(din, dout)
    rng = np.random.default_rng(5)
    g_out = rng.standard_normal((g.n, dout)).astype(np.float32)
    g_h = rng.standard_normal((g.n, dout)).astype(np.float32) if middle else None
    keep = None if p == 0 else R.keep_mask(R.SEED, 2, np.arange(g.n), dout, p)
    ref = R.layer_grads_torch(g, x, W1, W2, bias, R.SLOPE, keep, R.inv_keep32(p), g_out, g_h, torch.float64)
    cpu = R.layer_grads_torch(g, x, W1, W2, bias, R.SLOPE, keep, R.inv_keep32(p), g_out, g_h, torch.float32)

    def run():
        ts = [t32(t).to(DEV).requires_grad_() for t in (x, W1, W2, bias)]
        h, out = ops.NGCFLayerFn.apply(dev_csr(g), *ts, R.SLOPE, p, R.SEED, 2)
        loss = (out * t32(g_out).to(DEV)).sum()
        if middle:
            loss = loss + (h * t32(g_h).to(DEV)).sum()
        else:
            # the last layer's h has no gradient of its own: the entry takes g_h = NULL
            ds, dxd, dW1, dW2, db = ops.ngcf_layer_bwd(dev_csr(g), ts[0].detach(), ts[1].detach(), ts[2].detach(), h.detach(), t32(g_out).to(DEV),
                                                       None, R.SLOPE, p, R.SEED, 2)
            dx = dxd.clone()
            ops.graph_propagate(dev_csr(g), ds, sum=dx)
            return dict(zip(('dx', 'dW1', 'dW2', 'dbias'), (t.cpu() for t in (dx, dW1, dW2, db))))
        loss.backward()
        return dict(zip(('dx', 'dW1', 'dW2', 'dbias'), (t.grad.cpu() for t in ts)))

    before = ops.nondeterministic_launches()
    got, again = run(), run()
    assert ops.nondeterministic_launches() == before
    worst = []
    for k in ('dx', 'dW1', 'dW2', 'dbias'):
        _assert_bits(again[k], got[k], f'{k}: second run')
        e_cpu = L.yardstick(ref[k], cpu[k])
        err = float((got[k].double() - ref[k]).abs().max())
        print(f'{din} -> {dout} middle={middle} p={p} {k}: error {err:.3e}, float32 on the CPU {e_cpu:.3e}, allowed {L.FACTOR * e_cpu:.3e}')
        worst.append((k, err, L.FACTOR * e_cpu))
    for k, err, tol in worst:
        assert err <= tol, f'{k}: error {err:.3e} over 8 x the float32 CPU error = {tol:.3e}'


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    Sm = S()
    g = R.world(63, 64)
    n, din, dout = g.n, 8, 6
    W1n, W2n, bn = R.weights(din, dout)
    x, W1, W2 = _Buf(n, din, data=t32(L.table(n, din, 1))), _Buf(din, dout, data=t32(W1n)), _Buf(din, dout, data=t32(W2n))
    bias, h, out = _Buf(1, dout, data=t32(bn)[None]), _Buf(n, dout, fill=7.25), _Buf(n, dout + WIDE, fill=-3.5)
    big = _Buf(n, 129, fill=1.0)
    ds, dxd, go = _Buf(n, din, fill=7.25), _Buf(n, din, fill=7.25), _Buf(n, dout, fill=0.5)
    dW1, dW2, db = _Buf(din, dout, fill=7.25), _Buf(din, dout, fill=7.25), _Buf(1, dout, fill=7.25)
    ws = torch.zeros(1 << 16, device=DEV)

    def untouched():
        assert bool((h.check_untouched() == 7.25).all()) and bool((out.check_untouched() == -3.5).all())
        assert torch.equal(x.check_untouched(), t32(L.table(n, din, 1)))
        for b in (ds, dxd, dW1, dW2, db):
            assert bool((b.check_untouched() == 7.25).all())
        assert not bool(ws.any())

    def fwd(**kw):
        a = dict(x=x, W1=W1, W2=W2, bias=bias, h=h, out=out, din=din, dout=dout)
        a.update(kw)
        raw_fwd(g, a.pop('x'), a.pop('W1'), a.pop('W2'), a.pop('bias'), a.pop('h'), a.pop('out'), a.pop('din'), a.pop('dout'), **a)

    def bwd(**kw):
        a = dict(x=x.ptr, din=din, W1=W1.ptr, W2=W2.ptr, dout=dout, slope=R.SLOPE, p=0.0, h=h.ptr, go=go.ptr, ld=dout, gh=None, ds=ds.ptr, dxd=dxd.ptr,
                 dW1=dW1.ptr, dW2=dW2.ptr, db=db.ptr, ws=ws.data_ptr(), wsb=4 * ws.numel(), rows=(0, n))
        a.update(kw)
        call(BWD, *graph_args(g), a['rows'][0], a['rows'][1], a['x'], a['din'], a['W1'], a['W2'], a['dout'], float(a['slope']), float(a['p']), 1, 2,
             a['h'], a['go'], a['ld'], a['gh'], a['ds'], a['dxd'], a['dW1'], a['dW2'], a['db'], a['ws'], a['wsb'], stream())

    nan, inf = float('nan'), float('inf')
    for kw, text in (({'din': 0}, r'outside \[1, 128\]'), ({'din': 129, 'x': big}, r'outside \[1, 128\]'), ({'dout': 129, 'h': big}, r'outside \[1, 128\]'),
                     ({'dout': 0}, r'outside \[1, 128\]'), ({'rows': (0, n + 1)}, 'row range'), ({'rows': (3, 2)}, 'row range'), ({'rows': (-1, 2)}, 'row range'),
                     ({'ld': dout - 1}, 'out_ld=5 below Dout=6'), ({'slope': 0.0}, 'slope'), ({'slope': -0.5}, 'slope'), ({'slope': 1.5}, 'slope'),
                     ({'slope': nan}, 'slope'), ({'slope': inf}, 'slope'), ({'p': 1.0}, 'dropout rate'), ({'p': -0.1}, 'dropout rate'), ({'p': nan}, 'dropout rate'),
                     ({'h': x}, 'x aliases h'), ({'out_ptr': x.ptr, 'ld': din}, 'x aliases out'), ({'out_ptr': h.ptr, 'ld': dout}, 'h aliases out'),
                     ({'h': W1}, 'aliases h'), ({'out_ptr': bias.ptr, 'ld': dout}, 'aliases out')):
        with pytest.raises(Sm.SibrarHipError, match=text):
            fwd(**kw)
        untouched()
    for kw, text in (({'din': 129}, r'outside \[1, 128\]'), ({'rows': (0, n + 1)}, 'row range'), ({'ld': dout - 1}, 'out_ld'), ({'slope': nan}, 'slope'),
                     ({'p': 1.0}, 'dropout rate'), ({'ds': x.ptr}, 'x aliases ds'), ({'dxd': ds.ptr}, 'ds aliases dx_direct'), ({'dW1': W1.ptr}, 'W1 aliases dW1'),
                     ({'ds': go.ptr}, 'aliases ds'), ({'wsb': 64}, 'workspace of 64 bytes'), ({'ws': None}, 'workspace'),
                     ({'x': None}, 'null operand'), ({'h': None}, 'null operand'), ({'go': None}, 'null operand'), ({'db': None}, 'null operand')):
        with pytest.raises(Sm.SibrarHipError, match=text):
            bwd(**kw)
        untouched()
    for k in (0, 2, 8, 10, 11, 12, 18, 19):                                        # u_indptr, i_indptr, x, W1, W2, bias, h, out
        a = graph_args(g) + [0, n, x.ptr, din, W1.ptr, W2.ptr, bias.ptr, dout, R.SLOPE, 0.0, 1, 2, h.ptr, out.ptr, out.ld, stream()]
        a[k] = None
        with pytest.raises(Sm.SibrarHipError, match='null operand'):
            call(FWD, *a)
    untouched()
    fwd(rows=(4, 4))                                                               # an empty range is a no-op
    bwd(rows=(4, 4))
    untouched()
    # ops: a matrix with values, wrong tables
    csr = dev_csr(g)
    xs, w1, w2, b = x.t.contiguous(), W1.t.contiguous(), W2.t.contiguous(), bias.t[0].contiguous()
    weighted = g.m.copy()
    weighted.data[:] = 0.5
    with pytest.raises(ValueError, match='0/1'):
        Sm.ops.ngcf_layer(_mod('features').DeviceCSR(weighted).to(DEV), xs, w1, w2, b)
    for bad in ((xs[:-1], w1, w2, b), (xs.double(), w1, w2, b), (xs, w1.t().contiguous().t(), w2, b), (xs, w1, w2.double(), b), (xs, w1, w2, b[:-1]),
                (torch.empty(n, din + 1, device=DEV)[:, :din], w1, w2, b)):
        with pytest.raises(ValueError, match='contiguous float32'):
            Sm.ops.ngcf_layer(csr, *bad)
    with pytest.raises(ValueError, match='unit column stride'):
        Sm.ops.ngcf_layer(csr, xs, w1, w2, b, out=torch.empty(dout, n, device=DEV).t())
    with pytest.raises(ValueError, match='contiguous float32'):
        Sm.ops.ngcf_layer(csr, xs, w1, w2, b, h=torch.empty(n, dout + 1, device=DEV)[:, :dout])
    with pytest.raises(ValueError, match=r'outside \[1, 128\]'):
        Sm.ops.ngcf_layer(csr, torch.zeros(n, 129, device=DEV), torch.zeros(129, 4, device=DEV), torch.zeros(129, 4, device=DEV), torch.zeros(4, device=DEV))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Sm.ops.ngcf_layer(csr, xs.cpu(), w1, w2, b)
    hh = torch.zeros(n, dout, device=DEV)
    with pytest.raises(ValueError, match='contiguous float32'):
        Sm.ops.ngcf_layer_bwd(csr, xs, w1, w2, hh.double(), hh)
    with pytest.raises(ValueError, match='unit column stride'):
        Sm.ops.ngcf_layer_bwd(csr, xs, w1, w2, hh, hh.double())
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Sm.ops.ngcf_layer_bwd(csr, xs, w1, w2, hh, hh.cpu())
