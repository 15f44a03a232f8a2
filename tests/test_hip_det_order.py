"""GPU: deterministic mode's fixed-order kernels (csrc/deterministic.hip) against exact ORDER oracles, not tolerances.

  a. segmented row accumulation (``sbr_scatter_add_rows`` with the mode on; ``sbr_scatter_add_rows_det`` in either mode): bit for bit
     the numpy fp32 sum in ascending source position added once onto a PREFILLED table (tests/det_order_ref.py: scatter_in_order), at
     segment lengths on both sides of the 64-source split, every NC instantiation, second trips of both capped grids, probe chains and
     the wrap of the hash table, zero rows, n = 1 and n = 0; the sorted form of the data-parallel path gives the same bits;
  c. ``sbr_colsum`` in its fixed-slot form through the raw entry point: a bound derived from the launch geometry, stale scratch behind
     blocks with an empty row range, the refusals;
  d. ``sbr_csr_project_bwd_gather`` with the mode on: fixed-order up to C = 512, a named refusal above;
  e. the paths DESIGN.md §9 used to list as unpinned (tests/test_hip_det_paths.py holds the model-level half).
tests/test_det_order_cpu.py asserts on the CPU that every case reaches its branch and that the ladder is order sensitive."""
import numpy as np
import pytest
import torch

import det_order_ref as R
from hip_testutil import DEV, NAN, U32, S, _L, _assert_bits, _assert_bound, _Buf, _i32, _i64, _p, _rand, call, stream
from test_hip_tail import _err

pytestmark = pytest.mark.gpu
ENTRIES = (('sbr_scatter_add_rows', True), ('sbr_scatter_add_rows_det', False), ('sbr_scatter_add_rows_det', True))
NONE_WRITTEN = torch.zeros(0, dtype=torch.int64)


class _mode:
    """the switch set for a block, the counter reset; restored whatever happens"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.ops = S().ops
        self.prev = self.ops.set_deterministic(self.on)
        self.ops.nondeterministic_launches(reset=True)
        return self.ops

    def __exit__(self, *exc):
        self.ops.set_deterministic(self.prev)


_ORACLES = {}


def _oracle(c):
    if c.name not in _ORACLES:
        _ORACLES[c.name] = torch.from_numpy(c.oracle())
    return _ORACLES[c.name]


def _scatter(entry, c, dOut, dW, ii_d, rows_d):
    call(entry, dOut.ptr, dOut.ld, _p(ii_d), _p(rows_d), dW.ptr, dW.ld, c.n, c.D, stream())


# ---- a. segmented scatter -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', R.SCATTER_CASE_NAMES)
def test_segmented_scatter_equals_the_order_oracle(name):
    """Each entry point and mode on strided operands 4 bytes off a 16-byte boundary inside NaN guards: dW, prefilled with random nonzero
    values and some -0.0, equals the oracle in every bit (rows that no live source names keep theirs), the guards and the gradient rows
    are untouched, and the counter of arrival-order launches stays 0 — in default mode too: the _det entry point is fixed-order there."""
    c = R.scatter_case(name)
    want, g = _oracle(c), torch.from_numpy(c.g)
    for entry, on in ENTRIES:
        with _mode(on) as ops:
            dOut, dW = _Buf(g.shape[0], c.D, c.D + 4, 1, data=g), _Buf(c.n_table, c.D, c.D + 8, 1, data=torch.from_numpy(c.dW0))
            ii_d, rows_d = (None if c.ii is None else _i32(c.ii)), _i32(c.rows)
            _scatter(entry, c, dOut, dW, ii_d, rows_d)
            what = f'{entry} (deterministic={on}) {name}'
            _assert_bits(dW.check_untouched(None, what), want, what)
            _assert_bits(dOut.check_untouched(None, what + ' dOut'), g, what + ': the gradient rows changed')
            assert ops.nondeterministic_launches() == 0, what


def test_segmented_scatter_of_no_rows_is_a_no_op():
    for entry, on in ENTRIES:
        with _mode(on) as ops:
            call(entry, None, 0, None, None, None, 0, 0, 64, stream())
            dOut, dW = _Buf(1, 64), _Buf(1, 64)
            rows_d = _i32([0])
            call(entry, dOut.ptr, dOut.ld, None, _p(rows_d), dW.ptr, dW.ld, 0, 64, stream())
            dW.check_untouched(NONE_WRITTEN, entry + ' n = 0')
            assert ops.nondeterministic_launches() == 0


def test_sorted_form_gives_the_bits_of_the_segmented_form():
    """The data-parallel path's ``sbr_scatter_add_rows_sorted`` on the STABLE argsort of rows (one block: blk = n, block stride = n
    rows) adds the same rows in the same order: same bits as ``sbr_scatter_add_rows_det`` and as the oracle, on the ladder."""
    c = R.scatter_case('ladder')
    want, g = _oracle(c), torch.from_numpy(c.g)
    order = np.argsort(c.rows, kind='stable')
    perm_d, rs_d = _i64(c.ii[order]), _i32(c.rows[order])
    dOut, dW = _Buf(g.shape[0], c.D, c.D + 4, 1, data=g), _Buf(c.n_table, c.D, c.D + 8, 1, data=torch.from_numpy(c.dW0))
    call('sbr_scatter_add_rows_sorted', dOut.ptr, dOut.ld, c.n, c.n * dOut.ld, _p(perm_d), _p(rs_d), dW.ptr, dW.ld, c.n, c.D, stream())
    got_sorted = dW.check_untouched(None, 'sorted')
    dW2 = _Buf(c.n_table, c.D, c.D + 8, 1, data=torch.from_numpy(c.dW0))
    ii_d, rows_d = _i32(c.ii), _i32(c.rows)
    _scatter('sbr_scatter_add_rows_det', c, dOut, dW2, ii_d, rows_d)
    got_det = dW2.check_untouched(None, 'det')
    _assert_bits(got_sorted, got_det, 'sorted form vs segmented form')
    _assert_bits(got_sorted, want, 'sorted form vs the order oracle')


@pytest.mark.parametrize('D', [513, 0])
def test_segmented_scatter_refuses_rows_it_has_no_form_for(D):
    for entry, on in ENTRIES:
        with _mode(on):
            dOut, dW = _Buf(4, 520), _Buf(4, 520)
            rows_d = _i32([0, 1, 2, 3])
            msg = _err(entry, dOut.ptr, dOut.ld, None, _p(rows_d), dW.ptr, dW.ld, 4, D, stream())
            assert 'no deterministic form for rows of' in msg and msg.startswith(entry + ':'), msg
            dW.check_untouched(NONE_WRITTEN, entry + f' D = {D}')


# ---- c. sbr_colsum, fixed-slot form -------------------------------------------------------------------------------------------------
def _colsum(X, n, C, out, ws):
    call('sbr_colsum', X.ptr, X.ld, n, C, out.ptr, _p(ws), stream())
    return out.check_untouched(None, 'colsum')[0].clone()


@pytest.mark.parametrize('n,C,xl', R.COLSUM_CASES)
def test_fixed_slot_colsum_against_float64(n, C, xl, record_property):
    """out[c] = sum_j X[j, c] through the raw entry point with the mode on, X a strided view, the 17 C double workspace zeroed once.
    Bound, from the geometry (det_order_ref.col_reduce_geometry): a thread adds the rows lo + rl, lo + rl + RL, ... of its block in fp32,
    at most ceil(chunk / RL) of them, so at most that many additions (the four-way tree of the unrolled loop is no deeper than the
    chain); the lanes, the slots and the replicas are added in double (2^-53 per addition: far below u) and the total is rounded to fp32
    once: |err| <= (ceil(chunk / RL) + 2) u sum|x|. Two calls give the same bits, the replica part of the workspace is zero again and no
    arrival-order launch is counted. Before (4097, 1024) — 512 blocks of 9 rows, the last 56 without a row — a run of (8192, 1024) at
    1e6 leaves large sums in all 512 slots of the grow-only scratch: an empty block that skipped its store would fold them in."""
    with _mode(True) as ops:
        if (n, C) == R.COLSUM_EMPTY_TAIL:
            ns, Cs = R.COLSUM_STALE
            ws = torch.zeros(17 * Cs, dtype=torch.float64, device=DEV)
            big = _colsum(_Buf(ns, Cs, fill=1e6), ns, Cs, _Buf(1, Cs, off=1), ws)
            assert bool((big.double() == float(np.float32(ns * 1e6))).all())
        x = _rand(n, C, seed=n + C)
        X, out = _Buf(n, C, C + xl, 0, data=x), _Buf(1, C, off=1)
        ws = torch.zeros(17 * C, dtype=torch.float64, device=DEV)
        a = _colsum(X, n, C, out, ws)
        assert bool((ws[C:] == 0).all()), 'the replica part of the workspace is not left zeroed'
        out.flat.fill_(NAN)
        b = _colsum(X, n, C, out, ws)
        assert bool((ws[C:] == 0).all())
        _assert_bits(a, b, 'two calls of the fixed-slot column sum')
        ref, mag = x.double().sum(0), x.double().abs().sum(0)
        bound = (R.colsum_chain(n, C) + 2) * U32 * mag
        ratio = float(((a.double() - ref).abs() / bound).max())
        record_property('ratio_to_bound', ratio)
        print(f'colsum n={n} C={C}: chain {R.colsum_chain(n, C)}, worst |err| / bound = {ratio:.3f}')
        _assert_bound(a, ref, bound, f'fixed-slot colsum n={n} C={C}')
        assert ops.nondeterministic_launches() == 0


@pytest.mark.parametrize('C,xl,off', [(130, 0, 0), (1028, 0, 0), (64, 1, 0), (64, 0, 1)])
def test_fixed_slot_colsum_refuses_what_it_cannot_take(C, xl, off):
    """C % 4 != 0, C > 1024, ld % 4 != 0, a base pointer 4 bytes off: 'sbr_colsum: no deterministic form' and out untouched with the
    mode on; the same call runs in default mode (bound of test_hip_rowops.test_colsum_generic_branch), where the counter reads > 0."""
    n = 77
    x = _rand(n, C, seed=C + xl + off)
    X, out = _Buf(n, C, C + xl, off, data=x), _Buf(1, C, off=1)
    ws = torch.zeros(17 * C, dtype=torch.float64, device=DEV)
    with _mode(True) as ops:
        msg = _err('sbr_colsum', X.ptr, X.ld, n, C, out.ptr, _p(ws), stream())
        assert msg.startswith('sbr_colsum: no deterministic form'), msg
        out.check_untouched(NONE_WRITTEN, 'a refused sbr_colsum')
        assert bool((ws == 0).all()) and ops.nondeterministic_launches() == 0
    with _mode(False) as ops:
        got = _colsum(X, n, C, out, ws)
        ref = x.double().sum(0)
        _assert_bound(got, ref, U32 * ref.abs() + n * 2.0 ** -53 * x.double().abs().sum(0), 'colsum, default mode')
        assert ops.nondeterministic_launches() > 0


# ---- d. sbr_csr_project_bwd_gather ---------------------------------------------------------------------------------------------------
def _csr_world(C):
    """the construction of test_hip_rowops.test_csr_project_branches"""
    import scipy.sparse as sp
    rng = np.random.default_rng(C)
    n_rows, n_cols = 9, 40
    lens = [0, 1, 40, 7, 13, 0, 2, 33, 5]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(n_cols, size=l, replace=False)) for l in lens]).astype(np.int32)
    vals = rng.standard_normal(indices.size).astype(np.float32)
    mtx = sp.csr_matrix((vals, indices, indptr), shape=(n_rows, n_cols))
    dense = torch.from_numpy(mtx.toarray()).double()
    mt = mtx.T.tocsr()
    mt.sort_indices()
    rows = np.array([2, 0, 1, 2, 8, 7, 3, 4, 5, 6, 2])
    return n_rows, n_cols, dense, mt, rows


def _gather(C, world, dz):
    n_rows, n_cols, dense, mt, rows = world
    tp, tx, tv, rows_d = _i64(mt.indptr), _i32(mt.indices), torch.from_numpy(mt.data.astype(np.float32)).to(DEV), _i32(rows)
    dZ, dZe, dWt = _Buf(len(rows), C, C + 4, 0, data=dz), _Buf(n_rows, C), _Buf(n_cols, C, C + 8, 0, fill=0.25)
    args = (_p(tp), _p(tx), _p(tv), dZ.ptr, dZ.ld, None, _p(rows_d), len(rows), dZe.ptr, C, n_rows, dWt.ptr, dWt.ld, n_cols, C, stream())
    return args, dZe, dWt


def _gather_bound(C, world, dz):
    n_rows, n_cols, dense, mt, rows = world
    d = dense[torch.as_tensor(rows)]
    m = (d != 0).sum(0).double()[:, None]
    return d.t() @ dz.double() + 0.25, (m + 2) * U32 * (d.abs().t() @ dz.double().abs() + 0.25)


def test_csr_project_bwd_gather_is_fixed_order_up_to_512_columns():
    """C = 512 with the mode on: the (m + 2) u sum|terms| bound of test_csr_project_branches, two calls equal in bits, counter 0."""
    C = 512
    world, dz = _csr_world(C), _rand(11, C, seed=22)
    ref, bound = _gather_bound(C, world, dz)
    with _mode(True) as ops:
        seen = []
        for _ in range(2):
            args, dZe, dWt = _gather(C, world, dz)
            call('sbr_csr_project_bwd_gather', *args)
            dZe.check_untouched(None, 'workspace')
            seen.append(dWt.check_untouched(None, 'csr_project_bwd_gather'))
            _assert_bound(seen[-1], ref, bound, 'csr_project_bwd_gather, deterministic, C = 512')
        _assert_bits(seen[0], seen[1], 'two deterministic calls of sbr_csr_project_bwd_gather')
        assert ops.nondeterministic_launches() == 0


def test_csr_project_bwd_gather_refuses_wider_rows_loudly():
    """C = 516 (accepted by the entry point, which takes C <= 1024): its inner sbr_scatter_add_rows has no fixed-order form for rows of
    more than 512 floats, so with the mode on the call raises, naming that entry point and the width, and dWt keeps its bits; in default
    mode the same call meets the bound."""
    C = 516
    world, dz = _csr_world(C), _rand(11, C, seed=22)
    ref, bound = _gather_bound(C, world, dz)
    with _mode(True) as ops:
        args, dZe, dWt = _gather(C, world, dz)
        msg = _err('sbr_csr_project_bwd_gather', *args)
        assert 'sbr_scatter_add_rows: no deterministic form' in msg and '516 floats' in msg, msg
        _assert_bits(dWt.check_untouched(None, 'refused gather'), torch.full((40, C), 0.25), 'dWt of a refused call')
        assert ops.nondeterministic_launches() == 0
    with _mode(False) as ops:
        args, dZe, dWt = _gather(C, world, dz)
        call('sbr_csr_project_bwd_gather', *args)
        _assert_bound(dWt.check_untouched(None, 'csr_project_bwd_gather'), ref, bound, 'csr_project_bwd_gather, default mode, C = 516')
        assert ops.nondeterministic_launches() > 0
