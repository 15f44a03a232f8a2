"""The noisy propagation on the GPU: the entry 'sbr_graph_propagate_noise_f32' (csrc/graph_prop.hip) through the C ABI against its fp32
restatement bit for bit and against float64 inside the derived bound (tests/simgcl_ref.py), eps = 0 against 'sbr_graph_propagate_f32',
determinism over runs and row splits, the dependence on seed and stream_id, and the refusals.

Worlds (lightgcn_ref.world): 1 x 3 (the smallest), 5 x 64 (a user and an item without neighbours), 5 x 130 (users of degree 64 and 65:
a second trip of the group at every group size) and 257 x 3 (an item of degree 256). The widths cover both chunk widths, every
chunks-per-lane instantiation and every group size; where D % 4 == 0 the tables are also taken one float off the 16-byte boundary, which
forces the single-float kernels: the noise's summation order is a function of D alone, so the same restatement holds bit for bit."""
import numpy as np
import pytest
import torch

import lightgcn_ref as L
import simgcl_ref as R
from hip_testutil import DEV, S, _Buf, _assert_bits, _assert_bound, call, stream

pytestmark = pytest.mark.gpu
ENTRY, CLEAN = 'sbr_graph_propagate_noise_f32', 'sbr_graph_propagate_f32'
WORLDS = ((1, 3), (5, 64), (5, 130), (257, 3))
WIDTHS = (1, 3, 4, 5, 63, 64, 65, 128, 260, 512)
NEAR_CAP = 0.01                                # elements whose float64 p lies within its own bound of zero: at most 1% of a case

_WORLDS, _CSR = {}, {}


def dev_csr(g):
    if id(g) not in _CSR:
        from importlib import import_module
        _CSR[id(g)] = (g, import_module(S().ops.__name__.rsplit('.', 1)[0] + '.features').DeviceCSR(g.m).to(DEV))
    return _CSR[id(g)][1]


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def world(n_users, n_items):
    if (n_users, n_items) not in _WORLDS:
        _WORLDS[(n_users, n_items)] = L.world(n_users, n_items)
    return _WORLDS[(n_users, n_items)]


def raw(g, x, y, s, scale, d, eps, seed, sid, rows=None, entry=ENTRY):
    """the entry itself on _Buf operands (any alignment)"""
    csr = dev_csr(g)
    ti, tx, _ = csr.transposed()
    r0, r1 = (0, g.n) if rows is None else rows
    noise = (float(eps), int(seed), int(sid)) if entry == ENTRY else ()
    call(entry, csr.indptr.data_ptr(), csr.indices.data_ptr(), ti.data_ptr(), tx.data_ptr(), g.n_users, g.n_items, r0, r1, x.ptr, y.ptr,
         None if s is None else s.ptr, float(scale), d, *noise, stream())


def test_the_worlds_are_what_the_module_says():
    assert world(5, 64).deg[4] == 0 and world(5, 64).deg[5 + 2] == 0
    assert world(5, 130).deg[2] == 64 and world(5, 130).deg[3] == 65 and world(257, 3).deg[257] == 256


# ---- 1. the restatement bit for bit, float64 inside the bound, eps = 0, both chunk widths ------------------------------------------------
@pytest.mark.parametrize('d', WIDTHS)
@pytest.mark.parametrize('shape', WORLDS)
def test_noise_against_restatement_and_float64(shape, d):
    g = world(*shape)
    x, s0 = L.table(g.n, d, 1), L.table(g.n, d, 2)
    eps, seed, sid, scale = 0.1, 0x123456789ABCDEF0, R.stream_id(5, 1, 2) + (3 << 32), 1.0 / 3
    y_ref, s_ref = R.propagate_noise32(g, x, eps, seed, sid, s0, scale)
    y64 = R.propagate_noise64(g, x, eps, seed, sid)
    s64 = (s0.astype(np.float64) + y64) * float(np.float32(scale))
    by, bs, near, slack = R.propagate_noise_bound(g, x, eps, seed, sid, s0, scale)
    what = f'{shape[0]} x {shape[1]}, D = {d}'
    print(f'{what}: {int(near.sum())} of {near.size} elements within their bound of zero')
    assert near.mean() <= NEAR_CAP, f'{what}: {near.mean():.2%} of the elements may change sign, over the cap of 1%'
    bx, byy, bsum = _Buf(g.n, d, data=t32(x)), _Buf(g.n, d), _Buf(g.n, d, data=t32(s0))
    raw(g, bx, byy, bsum, scale, d, eps, seed, sid)
    y, acc = byy.check_untouched(what=what + ': y'), bsum.check_untouched(what=what + ': sum')
    _assert_bits(y, t32(y_ref), what + ': y against the restatement')
    _assert_bits(acc, t32(s_ref), what + ': sum against the restatement')
    _assert_bound(y, torch.from_numpy(y64), torch.from_numpy(by + near * slack), what + ': y against float64')
    _assert_bound(acc, torch.from_numpy(s64), torch.from_numpy(bs + near * slack * abs(scale)), what + ': sum against float64')
    assert torch.equal(bx.check_untouched(), t32(x))
    empty = torch.from_numpy(g.deg == 0)
    assert not bool(y[empty].any()) and not bool(torch.signbit(y[empty]).any()), what + ': a row without neighbours stays +0'
    p_ref = L.propagate32(g, x)[0]
    assert bool((y != t32(p_ref))[torch.from_numpy(p_ref != 0)].float().mean() > 0.9), what + ': the noise is there'
    # without a sum
    by2 = _Buf(g.n, d)
    raw(g, bx, by2, None, 1.0, d, eps, seed, sid)
    _assert_bits(by2.check_untouched(), t32(y_ref), what + ': y without a sum')
    # eps = 0: the bits of the clean entry, y and sum
    n0, ns0, c0, cs0 = _Buf(g.n, d), _Buf(g.n, d, data=t32(s0)), _Buf(g.n, d), _Buf(g.n, d, data=t32(s0))
    raw(g, bx, n0, ns0, scale, d, 0.0, seed, sid)
    raw(g, bx, c0, cs0, scale, d, None, None, None, entry=CLEAN)
    _assert_bits(n0.check_untouched(), c0.check_untouched(), what + ': eps = 0 against the clean entry')
    _assert_bits(ns0.check_untouched(), cs0.check_untouched(), what + ': eps = 0 against the clean entry: sum')
    _assert_bits(c0.host(), t32(p_ref), what + ': the clean entry')
    if d % 4 == 0:                                                            # one float off the boundary: the single-float kernels
        ox, oy, os_ = _Buf(g.n, d, off=1, data=t32(x)), _Buf(g.n, d, off=1), _Buf(g.n, d, off=1, data=t32(s0))
        raw(g, ox, oy, os_, scale, d, eps, seed, sid)
        _assert_bits(oy.check_untouched(what=what + ': y off the boundary'), t32(y_ref), what + ': y off the boundary')
        _assert_bits(os_.check_untouched(what=what + ': sum off the boundary'), t32(s_ref), what + ': sum off the boundary')


# ---- 2. determinism: runs, splits, rows outside the range; seed and stream_id ------------------------------------------------------------
@pytest.mark.parametrize('d', [3, 64, 65, 512])
def test_runs_and_row_splits_give_the_same_bits(d):
    g = world(257, 3)
    nu, n = g.n_users, g.n
    ops = S().ops
    x, s0 = t32(L.table(n, d, 1)).to(DEV), t32(L.table(n, d, 2)).to(DEV)
    eps, seed, sid = 0.2, 77, R.stream_id(9, 2, 3)
    acc = s0.clone()
    y = ops.graph_propagate_noise(dev_csr(g), x, eps, seed, sid, sum=acc, sum_scale=0.5)
    _assert_bits(y.cpu(), t32(R.propagate_noise32(g, x.cpu().numpy(), eps, seed, sid)[0]), 'ops against the restatement')
    acc_b = s0.clone()
    _assert_bits(ops.graph_propagate_noise(dev_csr(g), x, eps, seed, sid, sum=acc_b, sum_scale=0.5).cpu(), y.cpu(), 'second run')
    _assert_bits(acc_b.cpu(), acc.cpu(), 'second run: sum')
    for cuts in ([0, nu, n], [0, 1, 100, nu - 3, nu + 2, n - 1, n], [0, 0, 63, 64, 65, n]):
        out, acc_c = torch.full((n, d), 7.25, device=DEV), s0.clone()
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            before_y, before_s = out.clone(), acc_c.clone()
            ops.graph_propagate_noise(dev_csr(g), x, eps, seed, sid, out=out, sum=acc_c, sum_scale=0.5, rows=(r0, r1))
            keep = torch.ones(n, dtype=torch.bool, device=DEV)
            keep[r0:r1] = False
            assert torch.equal(out[keep], before_y[keep]) and torch.equal(acc_c[keep], before_s[keep]), f'rows outside [{r0}, {r1}) were written'
        _assert_bits(out.cpu(), y.cpu(), f'split {cuts}')
        _assert_bits(acc_c.cpu(), acc.cpu(), f'split {cuts}: sum')
    part = ops.graph_propagate_noise(dev_csr(g), x, eps, seed, sid, rows=(nu - 2, nu + 2))           # a new result: zeros outside the range
    assert torch.equal(part[nu - 2:nu + 2], y[nu - 2:nu + 2]) and not bool(part[:nu - 2].any()) and not bool(part[nu + 2:].any())
    # another seed, another stream_id (low and high half): another noise, each the restatement's
    clean = ops.graph_propagate(dev_csr(g), x)
    seen = [y.cpu()]
    for sd, st in ((seed + 1, sid), (seed + (1 << 32), sid), (seed, sid + 1), (seed, sid + (1 << 32))):
        other = ops.graph_propagate_noise(dev_csr(g), x, eps, sd, st).cpu()
        _assert_bits(other, t32(R.propagate_noise32(g, x.cpu().numpy(), eps, sd, st)[0]), f'seed {sd}, stream {st}')
        assert all(not torch.equal(other, o) for o in seen), f'seed {sd}, stream {st}: the same noise as before'
        seen.append(other)
    _assert_bits(ops.graph_propagate_noise(dev_csr(g), x, 0.0, seed, sid).cpu(), clean.cpu(), 'eps = 0 through ops')


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    Sm = S()
    g = world(5, 64)
    n, d = g.n, 8
    x, y, s = _Buf(n, d, data=t32(L.table(n, d, 1))), _Buf(n, d, fill=7.25), _Buf(n, d, fill=-3.5)
    wide = _Buf(n, 513, fill=1.0)

    def untouched():
        assert bool((y.check_untouched() == 7.25).all()) and bool((s.check_untouched() == -3.5).all())
        assert torch.equal(x.check_untouched(), t32(L.table(n, d, 1)))

    ok = (0.1, 1, 2)
    for args, text in (((g, x, x, s, 1.0, d, *ok), 'x aliases y'), ((g, x, y, x, 1.0, d, *ok), 'x aliases sum'),
                       ((g, x, y, y, 1.0, d, *ok), 'y aliases sum'), ((g, x, y, s, 1.0, 0, *ok), r'D=0 outside \[1, 512\]'),
                       ((g, wide, wide, None, 1.0, 513, *ok), r'D=513 outside \[1, 512\]'),
                       ((g, x, y, s, 1.0, d, *ok, (0, n + 1)), r'row range \[0, 70\) outside \[0, 69\]'),
                       ((g, x, y, s, 1.0, d, *ok, (3, 2)), 'row range'), ((g, x, y, s, 1.0, d, *ok, (-1, 2)), 'row range'),
                       ((g, x, y, s, 1.0, d, -0.1, 1, 2), 'eps'), ((g, x, y, s, 1.0, d, float('inf'), 1, 2), 'eps'),
                       ((g, x, y, s, 1.0, d, float('nan'), 1, 2), 'eps'), ((g, x, y, s, 1.0, d, -0.1, 1, 2, (4, 4)), 'eps')):
        with pytest.raises(Sm.SibrarHipError, match=ENTRY + '.*' + text):
            raw(*args)
        untouched()
    csr = dev_csr(g)
    ti, tx, _ = csr.transposed()
    for k in (0, 2, 8, 9):
        ptrs = [csr.indptr.data_ptr(), csr.indices.data_ptr(), ti.data_ptr(), tx.data_ptr(), 5, 64, 0, n, x.ptr, y.ptr, s.ptr, 1.0, d, 0.1, 1, 2,
                stream()]
        ptrs[k] = None
        with pytest.raises(Sm.SibrarHipError, match='null operand'):
            call(ENTRY, *ptrs)
        untouched()
    raw(g, x, y, s, 1.0, d, *ok, (4, 4))                                                  # an empty range is a no-op
    untouched()
    # ops: seed and stream_id outside 64 bits, a matrix with values, wrong tables, the host
    xs = x.t.contiguous()
    for seed, sid, text in ((-1, 0, 'seed'), (1 << 64, 0, 'seed'), (0, -1, 'stream_id'), (0, 1 << 64, 'stream_id'), (0.5, 0, 'seed')):
        with pytest.raises(ValueError, match=text):
            Sm.ops.graph_propagate_noise(csr, xs, 0.1, seed, sid)
    with pytest.raises(Sm.SibrarHipError, match='eps'):
        Sm.ops.graph_propagate_noise(csr, xs, -1.0, 0, 0)
    weighted = g.m.copy()
    weighted.data[:] = 0.5
    from importlib import import_module
    features = import_module(Sm.ops.__name__.rsplit('.', 1)[0] + '.features')
    with pytest.raises(ValueError, match='0/1'):
        Sm.ops.graph_propagate_noise(features.DeviceCSR(weighted).to(DEV), xs, 0.1, 0, 0)
    with pytest.raises(ValueError, match='contiguous float32'):
        Sm.ops.graph_propagate_noise(csr, xs[:-1], 0.1, 0, 0)
    with pytest.raises(Sm.SibrarHipError, match='x aliases y'):
        Sm.ops.graph_propagate_noise(csr, xs, 0.1, 0, 0, out=xs)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Sm.ops.graph_propagate_noise(csr, xs.cpu(), 0.1, 0, 0)
    untouched()
