"""GPU: sbr_rank_metrics_pos (csrc/topk.hip: dcg, ap, rr from one wave per user) through the C ABI against the references of
tests/rankpos_ref.py, whose header states the definitions, the kernel's float order and the derivation of the dcg bound;
tests/test_rank_pos_cpu.py proves the references on hand-worked lists and on the very inputs generated here.

  * ap and rr are divisions and additions of exactly converted integers: the kernel must return ``pos_metrics_f32`` bit for bit.
  * dcg goes through the device library's log2f, whose bits numpy need not share. It is checked twice: inside ``dcg_bound`` of the
    float64 definition, and bit for bit against the sum, in ascending hit order, of the device's OWN terms 1.f / log2f(r + 2), read off
    the entry itself on lists with a single hit at rank r (``device_terms``). The second check pins the order of the additions and
    leaves log2f free.
  * Lists and outputs live in NaN-filled guarded buffers (hip_testutil._Buf; the int32 lists through a bit view): a write outside the
    result fails the test, a read outside the list meets item 2,143,289,344."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import rankpos_ref as R
from hip_testutil import DEV, _L, _Buf, _bits, _i32, _i64, _p, call, stream

pytestmark = pytest.mark.gpu

ENTRY = 'sbr_rank_metrics_pos'


def _ibuf(data):
    """int32 [rows, cols] -> a guarded fp32 buffer holding the integers' bits"""
    data = torch.as_tensor(np.asarray(data), dtype=torch.int32)
    b = _Buf(data.shape[0], data.shape[1])
    b.t.view(torch.int32).copy_(data.to(DEV))
    return b


def _run(T, kmax, u_d, indptr, indices, Bu, ks, O, null=()):
    arr = (ctypes.c_int * len(ks))(*ks)
    args = {'topk': T.ptr, 'indptr': indptr.data_ptr(), 'indices': indices.data_ptr(), 'ks': ctypes.cast(arr, ctypes.c_void_p), 'out': O.ptr}
    args.update({name: None for name in null})
    call(ENTRY, args['topk'], kmax, _p(u_d), args['indptr'], args['indices'], Bu, args['ks'], len(ks), args['out'], stream())


def _metrics(top, u, csr, ks, what=''):
    """-> float32 [3, n_ks, Bu] as numpy, from guarded buffers; the lists must come back unchanged"""
    Bu, kmax = top.shape
    T, O = _ibuf(top), _Buf(3 * len(ks), Bu)
    _run(T, kmax, None if u is None else _i64(u), _i64(csr[0]), _i32(csr[1]), Bu, ks, O)
    assert torch.equal(_bits(T.check_untouched(None, f'{what} lists')), torch.as_tensor(top)), f'{what}: the lists changed'
    return O.check_untouched(None, what).numpy().reshape(3, len(ks), Bu).copy()


@functools.lru_cache(maxsize=None)
def device_terms():
    """float32 [300]: the device's 1.f / log2f(r + 2), as dcg@300 of a list whose only hit stands at rank r (0.f + term is the term)"""
    top, u, csr = R.single_hit_world(max(R.POS_KMAX))
    got = _metrics(top, u, csr, [max(R.POS_KMAX)], 'single-hit lists')
    want = R.pos_metrics_f32(top, u, csr, [max(R.POS_KMAX)])
    assert np.array_equal(got[1:].view(np.int32), want[1:].view(np.int32)), 'ap / rr of the single-hit lists'
    ref = R.pos_metrics_ref64(top, u, csr, [max(R.POS_KMAX)])[0, 0]
    assert (np.abs(got[0, 0] - ref) <= R.dcg_bound(top, u, csr, [max(R.POS_KMAX)])[0]).all(), 'a single term outside the bound'
    return got[0, 0].copy()


def _same_bits(got, want, what):
    diff = got.view(np.int32) != want.view(np.int32)
    assert not diff.any(), f'{what}: {int(diff.sum())} of {diff.size} values differ in bits, first at {np.argwhere(diff)[0].tolist()}'


@pytest.mark.parametrize('kmax', R.POS_KMAX)
@pytest.mark.parametrize('Bu', R.POS_BU)
def test_rank_metrics_pos_exact_and_inside_the_bound(Bu, kmax):
    terms, worst = device_terms(), 0.0
    for permuted in (False, True):
        top, u, csr = R.pos_world(Bu, kmax, permuted)
        for ks in R.pos_ks_sets(kmax):
            what = f'Bu {Bu} kmax {kmax} {"permuted" if permuted else "NULL u_idx"} ks {ks}'
            got = _metrics(top, u, csr, ks, what)
            assert not np.isnan(got).any(), f'{what}: an element was left unwritten'
            want = R.pos_metrics_f32(top, u, csr, ks, disc=terms)
            _same_bits(got[1], want[1], f'{what}: ap')
            _same_bits(got[2], want[2], f'{what}: rr')
            _same_bits(got[0], want[0], f'{what}: dcg against the ordered sum of the device\'s own terms')
            err, bound = np.abs(got[0] - R.pos_metrics_ref64(top, u, csr, ks)[0]), R.dcg_bound(top, u, csr, ks)
            assert (err <= bound).all(), f'{what}: dcg off by up to {err.max():.3e} (bound {bound[err.argmax() // Bu, err.argmax() % Bu]:.3e})'
            worst = max(worst, float((err / bound).max()))
            again = _metrics(top, u, csr, ks, what)
            _same_bits(again, got, f'{what}: a second run')
    print(f'dcg err / bound, worst over Bu {Bu} kmax {kmax}: {worst:.4f}')


def test_the_inputs_meet_every_branch():
    """asserted on the regenerated inputs of the test above, per list length over its user counts and both u_idx forms"""
    for kmax in R.POS_KMAX:
        met = set()
        for Bu in R.POS_BU:
            for permuted in (False, True):
                met |= R.branches_met(*R.pos_world(Bu, kmax, permuted))
        assert met >= R.branches_expected(kmax), f'kmax {kmax}: the inputs miss {sorted(R.branches_expected(kmax) - met)}'
        for k in (1, 64, 65, kmax):
            assert k > kmax or any(k in ks for ks in R.pos_ks_sets(kmax)), f'kmax {kmax}: no cut-off {k}'


def test_refusals_write_nothing():
    top, u, csr = R.pos_world(5, 65, False)
    T, indptr, indices = _ibuf(top), _i64(csr[0]), _i32(csr[1])
    err = _L().SibrarHipError
    for ks in ([], [1, 2, 3, 4, 5, 6, 7, 8, 9], [5, 3], [3, 3], [1, 66], [0, 4]):
        O = _Buf(3 * max(len(ks), 1), 5)
        with pytest.raises(err, match=ENTRY):
            _run(T, 65, None, indptr, indices, 5, ks, O)
        assert bool(torch.isnan(O.flat).all()), f'ks {ks}: a refused call wrote'
    for null in ('topk', 'indptr', 'indices', 'ks'):
        O = _Buf(3, 5)
        with pytest.raises(err, match=f'{ENTRY}: null operand'):
            _run(T, 65, None, indptr, indices, 5, [10], O, null=(null,))
        assert bool(torch.isnan(O.flat).all()), f'{null} NULL: a refused call wrote'
    O = _Buf(3, 5)
    with pytest.raises(err, match=f'{ENTRY}: null operand'):
        _run(T, 65, None, indptr, indices, 5, [10], O, null=('out',))
    O = _Buf(3, 5)
    _run(T, 65, None, indptr, indices, 0, [10], O)                # Bu = 0: nothing to do, no error
    assert bool(torch.isnan(O.flat).all())


def test_ops_wrapper_returns_the_entry_s_bits():
    from hip_testutil import S
    top, u, csr = R.pos_world(257, 130, True)
    ks = [1, 64, 65, 130]
    got = S().ops.rank_metrics_pos(torch.as_tensor(top).to(DEV), _i64(u), _i64(csr[0]), _i32(csr[1]), ks)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 4, 257)
    _same_bits(got.cpu().numpy(), _metrics(top, u, csr, ks, 'ops'), 'ops.rank_metrics_pos')
