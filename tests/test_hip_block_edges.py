"""The dense-block kernels (csrc/block128.h, als.hip, svd.hip, rbmf.hip, the tail of ease.hip) through the C ABI at the widths, slab
boundaries and staging edges where their code changes branch: sbr_rotate_cols_f32, sbr_col_residual_f32 and sbr_ease_weights_f32
(which only model fits reached before), sbr_gram_f32 / sbr_als_gram_f32 around their 512-row slabs, sbr_als_solve_rows_f32 on rows of
exactly 0, 1, 23, 24, 25, 47, 48, 49 and n_y entries, sbr_tri_solve_rows_f32 in place, sbr_chol_f32 at 63, 64 and 127.

Every operand lies in a NaN-filled guarded buffer with a leading dimension wider than the view and a base 4 bytes off; float
workspaces have guard bands too; inputs must come back unchanged and nothing outside the stated view may be written. The expected
values, the bounds and their derivations are in tests/block_ref.py (bit comparisons against exact integer arithmetic, everything else
float64 of the same fp32 inputs); tests/test_block_refs_cpu.py shows on the CPU that those checks pass the header's order and reject a
dropped or doubled slab row, exchanged columns 0 and 64, the row's diagonal, a missing floor and a scale applied before the chain.
Every figure is printed before it is asserted.

Worst error / bound measured on an MI355X: rotate 0.315, residual 0.249, Gram 0.015, ALS 0.187 of 8 x the yardstick,
triangular solve 0.080, Cholesky 0.077."""
import numpy as np
import pytest
import torch

import block_ref as B
from hip_testutil import DEV, GUARD, NAN, S, U32, _Buf, _assert_bits, _assert_bound, _i32, _i64, _L, _p, call

pytestmark = pytest.mark.gpu

assert U32 == B.U


class _Ws:
    """`need` bytes of fp32 workspace between two NaN guard bands"""

    def __init__(self, need):
        self.need, self.n = need, need // 4
        self.flat = torch.full((self.n + 2 * GUARD,), NAN, device=DEV)

    @property
    def ptr(self):
        return self.flat[GUARD:].data_ptr()

    def check(self, what):
        assert bool(torch.isnan(self.flat[:GUARD]).all()) and bool(torch.isnan(self.flat[GUARD + self.n:]).all()), f'{what}: written outside the workspace'


def _row(v, off=1):
    return _Buf(1, len(v), off=off, data=B.as_torch(v)[None, :])


def _same(buf, a, what):
    """the guarded input still holds its bits, and its surroundings their NaN"""
    _assert_bits(buf.check_untouched(what=what).contiguous(), B.as_torch(a).reshape(buf.rows, buf.cols), f'{what} was written')


def _np(buf, rows=None, what=''):
    return buf.check_untouched(rows, what=what).contiguous().numpy()


# ---- A. sbr_rotate_cols_f32 -----------------------------------------------------------------------------------------------------------
def run_rotate(Y, W, lam, in_place=False, tight=False):
    """raw sbr_rotate_cols_f32 -> (out [n, b], s [b] or None) on the host. s given lam NULL must keep its guard pattern."""
    n, b = Y.shape
    pad, off = (0, 0) if tight else (1, 1)
    yb = _Buf(n, b, ld=b + 3 * pad, off=off, data=B.as_torch(Y))
    wb = _Buf(b, b, ld=b + 5 * pad, off=off, data=B.as_torch(W))
    lb = None if lam is None else _row(lam, off)
    sb = _Buf(1, b, off=off)
    ob = yb if in_place else _Buf(n, b, ld=b + 2 * pad, off=3 * pad)
    call('sbr_rotate_cols_f32', yb.ptr, n, yb.ld, b, wb.ptr, wb.ld, None if lb is None else lb.ptr, sb.ptr, ob.ptr, ob.ld, _L().stream())
    _same(wb, W, 'W')
    if not in_place:
        _same(yb, Y, 'Y')
    if lam is None:
        sb.check_untouched(torch.zeros(1, dtype=torch.bool), what='s with lam NULL')
        return _np(ob, what='out'), None
    _same(lb, lam, 'lam')
    return _np(ob, what='out'), _np(sb, what='s')[0]


@pytest.mark.parametrize('n,b', B.ROT_CASES)
def test_rotate_cols_exact(n, b):
    Y, W = B.rotate_exact_inputs(n, b)
    for i, kind in enumerate(B.LAM_KINDS):
        lam = B.rotate_lam(b, kind, seed=n + b + i)
        out, s = run_rotate(Y, W, lam)
        B.check_rotate_exact(out, s, Y, W, lam)
    plain, _ = run_rotate(Y, W, None)
    B.check_rotate_exact(plain, None, Y, W, None)
    lam = B.rotate_lam(b, B.LAM_KINDS[0], seed=n + b)
    out, s = run_rotate(Y, W, lam)
    for what, kw in (('in place', {'in_place': True}), ('a second run on contiguous operands', {'tight': True}),
                     ('in place on contiguous operands', {'in_place': True, 'tight': True})):
        out2, s2 = run_rotate(Y, W, lam, **kw)
        B.same_bits(out2, out, what)
        B.same_bits(s2, s, what + ': s')
    B.same_bits(run_rotate(Y, W, None, in_place=True)[0], plain, 'in place, lam NULL')
    o_ops, s_ops = S().ops.rotate_cols(B.as_torch(Y).to(DEV), B.as_torch(W).to(DEV), B.as_torch(lam).to(DEV))
    B.same_bits(o_ops.cpu().numpy(), out, 'ops.rotate_cols')
    B.same_bits(s_ops.cpu().numpy(), s, 'ops.rotate_cols: s')
    B.same_bits(S().ops.rotate_cols(B.as_torch(Y).to(DEV), B.as_torch(W).to(DEV)).cpu().numpy(), plain, 'ops.rotate_cols, lam None')


@pytest.mark.parametrize('n,b', B.ROT_CASES)
def test_rotate_cols_float(n, b):
    Y, W, lam = B.rotate_float_inputs(n, b)
    out, s = run_rotate(Y, W, lam)
    ratio = B.check_rotate_float(out, s, Y, W, lam)
    print(f'rotate {n}x{b}: worst error / bound {ratio:.3f}')
    plain, _ = run_rotate(Y, W, None)
    Y64, W64 = B.as_torch(Y).double(), B.as_torch(W).double()
    _assert_bound(B.as_torch(plain), Y64 @ W64, b * U32 * (Y64.abs() @ W64.abs()), 'rotate, lam NULL')      # the chain's b roundings alone
    B.same_bits(run_rotate(Y, W, lam, in_place=True)[0], out, 'in place')


@pytest.mark.parametrize('b', [1, 65, 128])
def test_rotate_cols_without_rows_still_writes_s(b):
    """n = 0 with lam given: the header says s is written, the entry accepts null Y and out for n = 0 and launches one workgroup"""
    _, W = B.rotate_exact_inputs(1, b)
    lam = B.rotate_lam(b, B.LAM_KINDS[0], seed=b)
    wb, lb, sb, ob = _Buf(b, b, ld=b + 5, off=1, data=B.as_torch(W)), _row(lam), _Buf(1, b, off=1), _Buf(1, b, off=1)
    call('sbr_rotate_cols_f32', None, 0, b + 3, b, wb.ptr, wb.ld, lb.ptr, sb.ptr, None, b + 2, _L().stream())
    B.same_bits(_np(sb, what='s')[0], B.rotate_s32(lam), 's at n = 0')
    call('sbr_rotate_cols_f32', None, 0, b + 3, b, wb.ptr, wb.ld, lb.ptr, sb.ptr, ob.ptr, ob.ld, _L().stream())
    ob.check_untouched(torch.zeros(1, dtype=torch.bool), what='out at n = 0')
    _same(wb, W, 'W')
    _same(lb, lam, 'lam')


# ---- B. sbr_col_residual_f32 ----------------------------------------------------------------------------------------------------------
def run_residual(Y, Um, s, tight=False):
    n, f = Y.shape
    pad = 0 if tight else 1
    yb = _Buf(n, f, ld=f + 3 * pad, off=pad, data=B.as_torch(Y))
    ub = _Buf(n, f, ld=f + 6 * pad, off=pad, data=B.as_torch(Um))
    sb, rb = _row(s, pad), _Buf(1, f, off=pad)
    ws = _Ws(int(_L().lib().sbr_col_residual_f32_workspace(n, f)))
    assert ws.need == 4 * B.slabs(n, B.RES_SLAB) * f
    call('sbr_col_residual_f32', yb.ptr, yb.ld, ub.ptr, ub.ld, sb.ptr, n, f, rb.ptr, ws.ptr, ws.need, _L().stream())
    ws.check('col residual')
    _same(yb, Y, 'Y')
    _same(ub, Um, 'U')
    _same(sb, s, 's')
    return _np(rb, what='res')[0]


@pytest.mark.parametrize('n,f', B.RES_CASES)
def test_col_residual(n, f):
    for kind in ('zero', 'squares'):
        Y, Um, s, expected = B.col_residual_inputs(n, f, kind)
        B.check_col_residual_exact(run_residual(Y, Um, s), Y, Um, s, expected)
    for kind in ('float', 'cancel'):
        Y, Um, s, _ = B.col_residual_inputs(n, f, kind)
        res = run_residual(Y, Um, s)
        ratio = B.check_col_residual_float(res, Y, Um, s)
        print(f'col residual {n}x{f} {kind}: worst error / bound {ratio:.3f} (bound {B.col_residual_rel_bound(n):.2e} relative)')
        B.same_bits(run_residual(Y, Um, s, tight=True), res, 'a second run on contiguous operands')
        via = S().ops.col_residual(B.as_torch(Y).to(DEV), B.as_torch(Um).to(DEV), B.as_torch(s).to(DEV), f)
        B.same_bits(via.cpu().numpy(), res, 'ops.col_residual')


# ---- C. sbr_ease_weights_f32 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', B.EASE_N + (B.EASE_N_WRAP,))
def test_ease_weights(n):
    P = B.ease_inputs(n)
    pb, db = _Buf(n, n, ld=n + 3, off=1, data=B.as_torch(P)), _Buf(1, n, off=1)
    call('sbr_ease_weights_f32', pb.ptr, n, pb.ld, db.ptr, _L().stream())
    B.check_ease(_np(pb, what='P'), P)
    # the scratch: the header promises that the diagonal is read before it is overwritten; the code leaves the original diagonal there
    B.same_bits(_np(db, what='diag')[0], np.ascontiguousarray(np.diagonal(P)), 'diag scratch')


# ---- D. the Gram entries at slab edges ------------------------------------------------------------------------------------------------
def run_gram(entry, Y, n, f, *reg, tight=False):
    pad = 0 if tight else 1
    yb = None if n == 0 else _Buf(n, f, ld=f + 3 * pad, off=pad, data=B.as_torch(Y))
    gb = _Buf(f, f, ld=f + 5 * pad, off=pad)
    ws = _Ws(int(_L().lib().sbr_als_gram_f32_workspace(n, f)))
    assert ws.need == 4 * B.slabs(n, B.GRAM_SLAB) * f * f
    call(entry, None if yb is None else yb.ptr, n, f + 3 * pad, f, *reg, gb.ptr, gb.ld, ws.ptr if ws.need else None, ws.need, _L().stream())
    ws.check(entry)
    if yb is not None:
        _same(yb, Y, 'Y')
    return _np(gb, what=f'{entry} {n}x{f}')


@pytest.mark.parametrize('n,f', B.GRAM_CASES)
def test_gram_exact_at_slab_edges(n, f):
    Y = B.gram_inputs(n, f, 'int')
    plain = run_gram('sbr_gram_f32', Y, n, f)
    B.check_gram_exact(plain, Y)
    with_reg = run_gram('sbr_als_gram_f32', Y, n, f, B.GRAM_REG)
    B.check_gram_exact(with_reg, Y, B.GRAM_REG)
    B.same_bits(run_gram('sbr_gram_f32', Y, n, f, tight=True), plain, 'a second run on contiguous operands')
    B.same_bits(run_gram('sbr_als_gram_f32', Y, n, f, B.GRAM_REG, tight=True), with_reg, 'a second run on contiguous operands')


@pytest.mark.parametrize('n,f', B.GRAM_FLOAT_CASES)
def test_gram_float_at_slab_edges(n, f):
    Y = B.gram_inputs(n, f, 'float')
    r0 = B.check_gram_float(run_gram('sbr_gram_f32', Y, n, f), Y)
    r1 = B.check_gram_float(run_gram('sbr_als_gram_f32', Y, n, f, B.GRAM_REG), Y, B.GRAM_REG)
    print(f'gram {n}x{f}: worst error / bound {r0:.3f}, with reg {r1:.3f}')


@pytest.mark.parametrize('f', [1, 65, 128])
def test_als_gram_without_rows_is_reg_times_identity(f):
    got = run_gram('sbr_als_gram_f32', None, 0, f, B.GRAM_REG)
    B.same_bits(got, (np.eye(f, dtype=np.float32) * np.float32(B.GRAM_REG)).astype(np.float32), 'n_y = 0')


# ---- E. the row solvers at their staging edges ----------------------------------------------------------------------------------------
def run_solve(f, weighted, ranges=None, tight=False):
    (indptr, indices, data), (Y, G) = B.als_world(weighted), B.als_factors(f)
    n = len(indptr) - 1
    pad = 0 if tight else 1
    ops = [_i64(np.array(indptr)), _i32(np.array(indices)), None if data is None else B.as_torch(data).to(DEV)]
    yb = _Buf(B.ALS_NY, f, ld=f + 5 * pad, off=pad, data=B.as_torch(Y))
    out = _Buf(n, f, ld=f + 3 * pad, off=pad)
    gd = B.as_torch(G).to(DEV)
    info = torch.zeros(1, device=DEV, dtype=torch.int32)
    written = torch.zeros(n, dtype=torch.bool)
    for r0, r1 in ranges or [(0, n)]:
        call('sbr_als_solve_rows_f32', *[_p(o) for o in ops], r0, r1, yb.ptr, B.ALS_NY, yb.ld, f, _p(gd), B.ALS_ALPHA, out.ptr, out.ld, _p(info),
             _L().stream())
        written[r0:r1] = True
    assert int(info.item()) == 0, f'info = {int(info.item())}'
    _same(yb, Y, 'Y')
    assert torch.equal(gd.cpu(), B.as_torch(G)) and torch.equal(ops[1].cpu(), B.as_torch(indices))
    return out.check_untouched(written, what=f'solve rows {ranges}').contiguous().numpy()


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('f', B.ALS_F)
def test_als_solve_rows_at_the_staging_edges(f, weighted):
    got = run_solve(f, weighted)
    ratio = B.check_als(got, f, weighted)
    print(f'als solve f={f} weighted={weighted}: backward error / ({B.BACKWARD_FACTOR} x yardstick) {ratio:.3f}, yardstick '
          f'{B.als_yardstick(f, weighted):.3e}')
    n = len(B.ALS_ROW_NNZ)
    B.same_bits(run_solve(f, weighted, ranges=[(0, 4), (4, 5), (5, n)], tight=True), got, 'three ranges against one')
    part = run_solve(f, weighted, ranges=[(3, 7)])                                      # the rows of 23, 24, 25 and 47 entries alone
    B.same_bits(part[3:7], got[3:7], 'a range of its own')
    assert np.isnan(part[:3]).all() and np.isnan(part[7:]).all()


@pytest.mark.parametrize('r', B.TRI_R)
def test_tri_solve_rows_in_place(r):
    b, T = B.tri_inputs(r)
    n = B.TRI_N
    for upper in (0, 1):
        for unit in (0, 1):
            tb = _Buf(r, r, ld=r + 2, off=1, data=B.as_torch(T))                       # the other triangle and a unit diagonal are not read
            xin, xout = _Buf(n, r, ld=r + 5, off=1, data=B.as_torch(b)), _Buf(n, r, ld=r + 1, off=3)
            call('sbr_tri_solve_rows_f32', xin.ptr, xin.ld, n, r, tb.ptr, tb.ld, upper, unit, xout.ptr, xout.ld, _L().stream())
            _same(xin, b, 'in')
            x = _np(xout, what='out')
            ratio = B.check_tri(x, b, T, upper, unit)
            print(f'tri solve r={r} upper={upper} unit={unit}: worst residual / bound {ratio:.3f}')
            call('sbr_tri_solve_rows_f32', xin.ptr, xin.ld, n, r, tb.ptr, tb.ld, upper, unit, xin.ptr, xin.ld, _L().stream())
            B.same_bits(_np(xin, what='in place'), x, 'in place')
            _same(tb, T, 'T')


@pytest.mark.parametrize('n', B.CHOL_N)
def test_cholesky_at_the_wave_edges(n):
    K = B.chol_input(n)
    low = np.tril(K)                                                                # the lower triangle is read
    kb, rb = _Buf(n, n, ld=n + 3, off=1, data=B.as_torch(low)), _Buf(n, n, ld=n + 5, off=1)
    info = torch.zeros(1, device=DEV, dtype=torch.int32)
    call('sbr_chol_f32', kb.ptr, n, kb.ld, rb.ptr, rb.ld, _p(info), _L().stream())
    assert int(info.item()) == 0
    _same(kb, low, 'K')
    R = _np(rb, what='R')
    ratio = B.check_chol(R, K)
    print(f'cholesky n={n}: worst residual / bound {ratio:.3f}')
    B.same_bits(S().ops.cholesky(B.as_torch(low).to(DEV)).cpu().numpy(), R, 'ops.cholesky')
