"""'sbr_neumf_score_all' and 'sbr_neumf_score_pairs' (csrc/neumf.hip) through ops.neumf_score_all / ops.neumf_score_pairs: every pair's score
against float64 within the derived bound of tests/neumf_ref.py, with and without accumulate; row strides above the widths on all three
operands with NaN guard bands; dead ReLUs bit for bit; the same bits in one call, row by row, in item shards and through the pair list;
each operand in turn with a row that starts past 2^31 elements; the refusals."""
import numpy as np
import pytest
import torch

import neumf_ref as R
from hip_testutil import DEV, S, _assert_bits

pytestmark = pytest.mark.gpu


def _ops():
    return S().ops


def _dev(c):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t(c['A']), t(c['Bt']), t(R.pack_tail(c)), t(c['base'])


@pytest.mark.parametrize('widths', R.TAILS)
@pytest.mark.parametrize('accumulate', [False, True])
def test_scores_against_float64_within_the_bound(widths, accumulate):
    worst = 0.
    for Bu in R.BUS:
        for I in R.IS:
            c = R.kernel_case(Bu, I, widths)
            A, Bt, tail, base = _dev(c)
            got = _ops().neumf_score_all(A, Bt, tail, widths, out=base.clone() if accumulate else None, accumulate=accumulate)
            want, bound = R.truth_and_bound(c, accumulate)
            ratio = float(((got.double().cpu() - want).abs() / bound).max())
            worst = max(worst, ratio)
            assert got.shape == (Bu, I) and ratio <= 1., (Bu, I, widths, accumulate, ratio)
    print(f'widths {widths}, accumulate {accumulate}: largest error / bound {worst:.3f}')


@pytest.mark.parametrize('widths', [(5,), (32, 16, 8)])
def test_row_strides_above_the_widths_and_nan_guard_bands(widths):
    Bu, I, h1 = 65, 130, widths[0]
    c = R.kernel_case(Bu, I, widths)
    A, Bt, tail, base = _dev(c)
    want = _ops().neumf_score_all(A, Bt, tail, widths)
    nan = float('nan')
    Ab, Bb = torch.full((Bu, h1 + 3), nan, device=DEV), torch.full((I, h1 + 7), nan, device=DEV)
    Ab[:, 1:1 + h1], Bb[:, 2:2 + h1] = A, Bt
    flat = torch.full((5 + Bu * (I + 9) + 5,), nan, device=DEV)
    out = flat[5:5 + Bu * (I + 9)].view(Bu, I + 9)[:, :I]
    got = _ops().neumf_score_all(Ab[:, 1:1 + h1], Bb[:, 2:2 + h1], tail, widths, out=out)
    assert got.data_ptr() == out.data_ptr()
    _assert_bits(got.cpu(), want.cpu(), 'strided operands')
    band = torch.ones_like(flat, dtype=torch.bool)
    band[5:5 + Bu * (I + 9)].view(Bu, I + 9)[:, :I] = False
    assert bool(torch.isnan(flat[band]).all()), 'the guard bands around out and between its rows are untouched'
    out.copy_(base)
    _ops().neumf_score_all(Ab[:, 1:1 + h1], Bb[:, 2:2 + h1], tail, widths, out=out, accumulate=True)
    _assert_bits(out.cpu(), _ops().neumf_score_all(A, Bt, tail, widths, out=base.clone(), accumulate=True).cpu(), 'strided, accumulate')
    assert bool(torch.isnan(flat[band]).all())


@pytest.mark.parametrize('widths', R.TAILS)
def test_all_relus_dead_gives_c_bit_for_bit(widths):
    c = R.kernel_case(65, 130, widths, dead=True)
    A, Bt, tail, base = _dev(c)
    cc = torch.from_numpy(c['c']).to(DEV)
    _assert_bits(_ops().neumf_score_all(A, Bt, tail, widths).cpu(), cc.expand(65, 130).cpu(), 'c')
    got = _ops().neumf_score_all(A, Bt, tail, widths, out=base.clone(), accumulate=True)
    _assert_bits(got.cpu(), (base + cc).cpu(), 'fl(base + c)')


@pytest.mark.parametrize('widths', [(5,), (3, 2), (32, 16, 8), (64, 64, 64, 64)])
def test_tile_invariance_and_repeatability(widths):
    Bu, I = 65, 130
    c = R.kernel_case(Bu, I, widths)
    A, Bt, tail, base = _dev(c)
    f = _ops().neumf_score_all
    whole = f(A, Bt, tail, widths)
    _assert_bits(f(A, Bt, tail, widths).cpu(), whole.cpu(), 'a second call')
    rows = torch.cat([f(A[r:r + 1], Bt, tail, widths) for r in range(Bu)])
    _assert_bits(rows.cpu(), whole.cpu(), 'row by row')
    for lo, hi in ((0, 64), (64, 130), (17, 130)):
        _assert_bits(f(A, Bt[lo:hi], tail, widths).cpu(), whole[:, lo:hi].cpu(), f'items [{lo}, {hi})')
    u_slot = torch.arange(Bu, device=DEV).repeat_interleave(I)
    i_slot = torch.arange(I, device=DEV).repeat(Bu)
    perm = torch.randperm(Bu * I, generator=torch.Generator().manual_seed(1)).to(DEV)
    pairs = _ops().neumf_score_pairs(A, Bt, u_slot[perm], i_slot[perm], tail, widths)
    _assert_bits(pairs.cpu(), whole.reshape(-1)[perm].cpu(), 'the pair list')
    acc = _ops().neumf_score_pairs(A, Bt, u_slot, i_slot, tail, widths, out=base.reshape(-1).clone(), accumulate=True)
    _assert_bits(acc.cpu(), f(A, Bt, tail, widths, out=base.clone(), accumulate=True).reshape(-1).cpu(), 'the pair list, accumulate')
    bad = _ops().neumf_score_pairs(A, Bt, torch.tensor([0, Bu, -1, 0], device=DEV), torch.tensor([I, 0, 0, 1], device=DEV), tail, widths)
    assert torch.isnan(bad[:3]).all() and float(bad[3]) == float(whole[0, 1]), 'a slot outside its matrix gives a NaN'


def test_rows_past_2_to_31_elements_on_each_operand():
    """One 8 GiB buffer, nothing filled, serves in turn as ``out``, as ``A`` and as ``Bt`` with a row stride past 2^31 elements, so that row 1
    starts beyond element 2^31; the other operands are compact. Each result has the bits of the all-compact call."""
    widths, I, h1 = (5,), 65, 5
    ld = 2 ** 31 + 24
    c = R.kernel_case(2, I, widths)
    A, Bt, tail, base = _dev(c)
    f = _ops().neumf_score_all
    want = f(A, Bt, tail, widths)
    try:
        flat = torch.empty(ld + I, device=DEV, dtype=torch.float32)
    except RuntimeError as e:                                     # 8 GiB
        pytest.skip(f'no room for a buffer of {4 * (ld + I) / 2 ** 30:.1f} GiB: {e}')
    try:
        out = flat.as_strided((2, I), (ld, 1))
        probe = [I, I + 1, 2 ** 31 - 1, 2 ** 31, ld - 1]          # the band before row 1, sampled
        flat[probe] = 7.
        got = f(A, Bt, tail, widths, out=out)
        _assert_bits(got.cpu(), want.cpu(), 'stride_o past 2^31')
        assert flat[probe].cpu().tolist() == [7.] * len(probe), 'the band before row 1 is untouched where sampled'
        big = flat.as_strided((2, h1), (ld, 1))
        big.copy_(A)
        _assert_bits(f(big, Bt, tail, widths).cpu(), want.cpu(), 'stride_a past 2^31')
        big.copy_(Bt[3:5])
        _assert_bits(f(A, big, tail, widths).cpu(), want[:, 3:5].cpu(), 'stride_b past 2^31')
        pairs = _ops().neumf_score_pairs(A, big, torch.tensor([1, 0, 1], device=DEV), torch.tensor([1, 1, 0], device=DEV), tail, widths)
        _assert_bits(pairs.cpu(), torch.stack([want[1, 4], want[0, 4], want[1, 3]]).cpu(), 'the pair list, stride_b past 2^31')
    finally:
        del flat, out
        torch.cuda.empty_cache()


def test_refusals_launch_nothing():
    ops = _ops()
    lib = __import__('importlib').import_module(ops.__name__.rsplit('.', 1)[0] + '._lib')
    z = lambda *s: torch.zeros(*s, device=DEV)
    lib.CALL_LOG = []
    try:
        for widths, h1 in (((65,), 65), ((8, 65), 8), ((8,) * 5, 8), ((), 8)):
            with pytest.raises(ValueError):
                ops.neumf_score_all(z(3, h1), z(4, h1), z(max(ops.neumf_tail_len(widths) if widths else 1, 1)), widths)
        with pytest.raises(ValueError):
            ops.neumf_score_all(z(3, 8), z(4, 7), z(ops.neumf_tail_len((8, 4))), (8, 4))              # Bt narrower than H1
        with pytest.raises(ValueError):
            ops.neumf_score_all(z(3, 8), z(4, 8), z(ops.neumf_tail_len((8, 4)) + 1), (8, 4))          # a tail of the wrong length
        with pytest.raises(ValueError):
            ops.neumf_score_all(z(3, 8).double(), z(4, 8), z(ops.neumf_tail_len((8, 4))), (8, 4))
        with pytest.raises(ValueError):
            ops.neumf_score_all(z(8, 3).t(), z(4, 8), z(ops.neumf_tail_len((8, 4))), (8, 4))          # columns, not rows, contiguous
        with pytest.raises(ValueError):
            ops.neumf_score_all(z(3, 8), z(4, 8), z(ops.neumf_tail_len((8, 4))), (8, 4), accumulate=True)
        with pytest.raises(ValueError):
            ops.neumf_score_all(z(3, 8), z(4, 8), z(ops.neumf_tail_len((8, 4))), (8, 4), out=z(3, 5))
        with pytest.raises(RuntimeError):
            ops.neumf_score_all(torch.zeros(3, 8), z(4, 8), z(ops.neumf_tail_len((8, 4))), (8, 4))
        empty = ops.neumf_score_all(z(0, 8), z(4, 8), z(ops.neumf_tail_len((8, 4))), (8, 4))
        assert empty.shape == (0, 4)
        assert ops.neumf_score_all(z(3, 8), z(0, 8), z(ops.neumf_tail_len((8, 4))), (8, 4)).shape == (3, 0)
        assert [n for n, _ in lib.CALL_LOG] == [], 'nothing reached the library'
        # the library's own checks, past the Python front
        tail = z(ops.neumf_tail_len((8, 4)))
        for args in ((5, 8, 4, 0, 0), (2, 65, 4, 0, 0), (2, 8, 0, 0, 0)):
            with pytest.raises(lib.SibrarHipError):
                lib.call('sbr_neumf_score_all', z(3, 8).data_ptr(), 8, z(4, 8).data_ptr(), 8, tail.data_ptr(), tail.numel(), *args,
                         z(3, 4).data_ptr(), 4, 3, 4, 0, lib.stream())
        # more than 2^24 workgroups of 32 users x 64 items: refused with the advice to chunk, before any launch (the pointers are never read)
        a, b, o = z(3, 8), z(4, 8), z(3, 4)
        with pytest.raises(lib.SibrarHipError, match='chunks'):
            lib.call('sbr_neumf_score_all', a.data_ptr(), 8, b.data_ptr(), 8, tail.data_ptr(), tail.numel(), 2, 8, 4, 0, 0, o.data_ptr(),
                     1088, 32 * 2 ** 20, 1088, 0, lib.stream())
        with pytest.raises(lib.SibrarHipError, match='chunks'):
            lib.call('sbr_neumf_score_pairs', a.data_ptr(), 8, 3, b.data_ptr(), 8, 4, o.data_ptr(), o.data_ptr(), tail.data_ptr(),
                     tail.numel(), 2, 8, 4, 0, 0, o.data_ptr(), 1024 * 2 ** 24 + 1, 0, lib.stream())
    finally:
        lib.CALL_LOG = None
    torch.cuda.synchronize()
