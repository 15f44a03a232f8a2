"""Address arithmetic past 2^31 and 2^32 elements in the row-addressed table kernels (csrc/rowops.hip: gather, lookup, scatter-add,
bag mean, CSR project) and in the two entries that work on the evaluation score matrix (sbr_floor_scores, sbr_uniform_rows_f32). The
table kernels form ``rows[j] * ldw`` with rows[j] an int read from memory: an embedding table of 33.6 M rows x 64 columns is past 2^31
elements, and a 130-row view at a large stride gives the same products. The scheme of tests/test_hip_big_ld.py: one operand of each
call is a view of 130 rows at LD_BIG = 2^25 + 64 inside the one untouched 16.1 GiB buffer, everything else is compact; every operand
that has a leading dimension gets LD_BIG in a case of its own.

Each case asserts (a) the entry's float64 reference under the bound of its own test module (tests/rowops_ref.py, det_order_ref.py,
evalk_ref.py, naive_ref.py; nothing new), (b) bit equality with the same call at ld = 192, (c) the guard bands: inputs keep their
bits, and in the tables written by row (dW, dWt, out under out_idx) every row that no index names holds its bits from before the call
across the full width.

Index vectors (rows, in_idx, out_idx, dz_idx, perm, rows_sorted, tags, the CSR indices) are permutations or draws that name rows 0,
63, 64, 65, 127, 128, 129 of the big operand (asserted before the call); the optional ones are NULL in one case and given in another.
D and C in {5, 64, 128}: the scalar kernels, the float4 kernels, and with n = 4100 the 128-wide persistent scatter kernel.

sbr_scatter_add_rows, sbr_bag_mean_bwd, sbr_csr_project_bwd (and sbr_csr_project_bwd_gather, which scatters into its workspace first)
add with float atomics in arrival order: their inputs are small integers, halves and quarters whose sums stay far below 2^24, so every
order of addition gives the same bits (checked on the CPU first: np.add.at forwards and backwards equals the float64 reference).

Operands that reach no crossing: dZe [n_entities, C] of sbr_csr_project_bwd_gather must be dense (lde = C is required by the entry);
the entry is tested through dZ and dWt. sbr_lookup_rows and sbr_csr_project_bwd_gather take no D = 5 (D % 4 != 0 is refused)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import det_order_ref
import evalk_ref as E
import naive_ref
import rowops_ref as RR
from big_ld_util import EDGE_ROWS, N, both, compact, covers, draw_rows, out, perm_rows, some_rows, unchanged
from hip_testutil import DEV, _BigLd, _assert_bits, _assert_bound, _bits, _i32, _i64, _L, _p, _rand, call

pytestmark = pytest.mark.gpu

DS = (5, 64, 128)
DS4 = (64, 128)


@pytest.fixture(scope='module', autouse=True)
def big_buffer():
    """the one large allocation of the module (skips the module when the device has no room for it), freed at the end"""
    _BigLd._flat()
    torch.cuda.reset_peak_memory_stats()
    yield
    print(f'peak device memory of the module: {torch.cuda.max_memory_allocated()} bytes')
    _BigLd.release()


def _pick(which, make, *names):
    return [(make if which == w else compact) for w in names]


def _ints(n, D, seed, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, (n, D), generator=torch.Generator().manual_seed(seed)).float()


def _orders_agree(dst, terms, n_table, ref, what):
    """the premise of an atomic case: the fp32 sums per destination row, added forwards and backwards, equal the float64 reference"""
    dst, terms = np.asarray(dst, dtype=np.int64), np.asarray(terms, dtype=np.float32)
    fwd, bwd = (np.zeros((n_table, terms.shape[1]), dtype=np.float32) for _ in range(2))
    np.add.at(fwd, dst, terms)
    np.add.at(bwd, dst[::-1], terms[::-1])
    want = ref.float().numpy()
    assert np.array_equal(want.astype(np.float64), ref.numpy()), f'{what}: the reference is not representable in fp32'
    assert np.array_equal(fwd, want) and np.array_equal(bwd, want), f'{what}: the inputs do not sum to the same bits in every order'


def _named(rows):
    return np.unique(np.asarray(rows))


# ---- sbr_gather_rows, sbr_lookup_rows(_supported) ------------------------------------------------------------------------------------
@pytest.mark.parametrize('idx', [False, True], ids=['no out_idx', 'out_idx'])
@pytest.mark.parametrize('which', ['W', 'out'])
@pytest.mark.parametrize('D', DS)
def test_gather_rows(D, which, idx):
    """out[oi(j), :] = W[rows[j], :] bit for bit. W [130, D] under rows (a draw with repeats); out [130, D], under out_idx 120 slots into
    its 130 rows"""
    n = 120 if idx else N
    w = _rand(N, D, seed=D)
    rows = draw_rows(n, 20 + D)
    oi = some_rows(n, 21 + D) if idx else None
    rows_d, oi_d = _i32(rows), None if oi is None else _i32(oi)
    what = f'sbr_gather_rows D={D} {which}'

    def run(make):
        mw, mo = _pick(which, make, 'W', 'out')
        Wb, Ob = mw(N, D, w), mo(N, D)
        call('sbr_gather_rows', Wb.ptr, Wb.ld, _p(rows_d), Ob.ptr, Ob.ld, _p(oi_d), n, D, _L().stream())
        unchanged(Wb, w, 'W')
        return out(Ob, np.arange(n) if oi is None else oi, what=what)

    got = both(run, what)
    dst = torch.as_tensor(np.arange(n) if oi is None else oi)
    _assert_bits(got[dst], w[torch.as_tensor(rows)], what)


def _lookup_world(n_ids=150):
    """ids -> rows through a map with holes: 130 of the 150 ids have a row (a permutation of the 130 table rows), 20 map to -1"""
    rng = np.random.default_rng(77)
    rowmap = np.full(n_ids, -1, dtype=np.int64)
    have = rng.permutation(n_ids)[:N]
    rowmap[have] = rng.permutation(N)
    return rowmap, have


@pytest.mark.parametrize('which', ['W', 'out'])
@pytest.mark.parametrize('D', DS4)
def test_lookup_rows(D, which):
    """sbr_lookup_rows_supported answers the same at LD_BIG and at 192 (1 for D = 64 / 128, 0 for D = 5 at either), and sbr_lookup_rows
    then gives rows_out and the bits of the gather route (sbr_gather_rows on rows_out). A second call holds an id that the map rejects:
    err_flag is set, the slot reads row 0, and nothing past the view is written."""
    rowmap, have = _lookup_world()
    w = _rand(N, D, seed=30 + D)
    ids_ok = np.random.default_rng(D).permutation(have)                 # every table row once: covers the edge rows
    covers(rowmap[ids_ok], 'rowmap[idx]')
    ids_bad = ids_ok.copy()
    ids_bad[[5, 64, 129]] = [int(np.flatnonzero(rowmap < 0)[0]), -1, len(rowmap) + 3]
    map_d = _i32(rowmap)
    what = f'sbr_lookup_rows D={D} {which}'
    supported = getattr(_L().lib(), 'sbr_lookup_rows_supported')

    def run(make):
        mw, mo = _pick(which, make, 'W', 'out')
        res = []
        for ids, bad in ((ids_ok, False), (ids_bad, True)):
            Wb, Ob, Gb = mw(N, D, w), mo(N, D), compact(N, D)       # (one big view at a time: the gather route writes a compact out)
            assert int(supported(Wb.ptr, Wb.ld, Ob.ptr, Ob.ld, D)) == 1
            assert int(supported(Wb.ptr, Wb.ld, Ob.ptr, Ob.ld, 5)) == 0
            ids_d = _i64(ids)
            rows_out, err = torch.full((N + 8,), -7, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
            call('sbr_lookup_rows', _p(ids_d), N, _p(map_d), len(rowmap), Wb.ptr, Wb.ld, _p(rows_out), Ob.ptr, Ob.ld, D, _p(err), _L().stream())
            assert int(err) == int(bad) and rows_out[N:].cpu().tolist() == [-7] * 8
            unchanged(Wb, w, 'W')
            got = out(Ob, what=what)
            call('sbr_gather_rows', Wb.ptr, Wb.ld, _p(rows_out), Gb.ptr, Gb.ld, None, N, D, _L().stream())
            _assert_bits(got, out(Gb, what='the gather route'), what + ' against the gather route')
            res += [got, rows_out[:N].cpu()]
        return tuple(res)

    got_ok, rows_ok, got_bad, rows_bad = both(run, what)
    want_ok = rowmap[ids_ok]
    inside = (ids_bad >= 0) & (ids_bad < len(rowmap))
    want_bad = np.where(inside, rowmap[np.clip(ids_bad, 0, len(rowmap) - 1)], -1)
    assert int((want_bad < 0).sum()) == 3
    want_bad = np.maximum(want_bad, 0)
    assert rows_ok.tolist() == want_ok.tolist() and rows_bad.tolist() == want_bad.tolist()
    _assert_bits(got_ok, w[torch.as_tensor(want_ok)], what)
    _assert_bits(got_bad, w[torch.as_tensor(want_bad)], what + ' with rejected ids')


def test_lookup_rows_refuses_d5_at_either_ld():
    w = _rand(N, 5, seed=1)
    ids_d, err, rows_out = _i64(np.arange(N)), torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV)
    for make in (lambda r, c, d=None: _BigLd(r, c, data=d), compact):
        Wb, Ob = make(N, 5, w), compact(N, 5)
        with pytest.raises(_L().SibrarHipError):
            call('sbr_lookup_rows', _p(ids_d), N, None, N, Wb.ptr, Wb.ld, _p(rows_out), Ob.ptr, Ob.ld, 5, _p(err), _L().stream())
        out(Ob, [], what='refused sbr_lookup_rows')
        unchanged(Wb, w, 'W')


# ---- sbr_scatter_add_rows, _det, _sorted ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('idx', [False, True], ids=['no in_idx', 'in_idx'])
@pytest.mark.parametrize('which', ['dOut', 'dW'])
@pytest.mark.parametrize('D', DS)
def test_scatter_add_rows(D, which, idx):
    """dW[rows[j], :] += dOut[ii(j), :] with float atomics into a zeroed table: integer gradient rows in {-3..3} (every order of addition
    gives the same bits; sums <= 3 n < 2^24). rows is a draw with repeats in which rows 64, 128 and 129 are named more than once, so the
    atomics land past both wraps several times. With in_idx, n = 4100 sources drawn from the 130 rows of dOut: at D = 128 that is the
    persistent 128-wide kernel (n >= 4096), otherwise the power-of-two (64, 128) and grid-stride (5) kernels. The bound of
    tests/test_hip_rowops.py::test_scatter_add_rows (m u sum|terms|), and, the inputs being exact, equality with the reference."""
    n = 4100 if idx else N
    g = _ints(N, D, 40 + D)
    rows = draw_rows(n, 41 + D)
    rows[:6], rows[6:13] = [64, 64, 128, 128, 129, 129], EDGE_ROWS
    assert all(int((rows == r).sum()) > 1 for r in (64, 128, 129))
    covers(rows, 'rows')
    ii = draw_rows(n, 42 + D) if idx else None
    ref, bound, m = RR.scatter_add_ref(g, ii, rows, N)
    _orders_agree(rows, g[torch.as_tensor(np.arange(n) if ii is None else ii)].numpy(), N, ref, 'sbr_scatter_add_rows')
    rows_d, ii_d = _i32(rows), None if ii is None else _i32(ii)
    what = f'sbr_scatter_add_rows D={D} {which} n={n}'

    def run(make):
        mo, mw = _pick(which, make, 'dOut', 'dW')
        Ob, Wb = mo(N, D, g), mw(N, D, fill=0.0)
        call('sbr_scatter_add_rows', Ob.ptr, Ob.ld, _p(ii_d), _p(rows_d), Wb.ptr, Wb.ld, n, D, _L().stream())
        unchanged(Ob, g, 'dOut')
        return out(Wb, _named(rows), what=what)

    got = both(run, what)
    _assert_bound(got, ref, bound, what)
    assert torch.equal(got.double(), ref), what
    assert bool((_bits(got[m[:, 0] == 0]) == 0).all()), 'a table row that no source names was written'


@pytest.mark.parametrize('idx', [False, True], ids=['no in_idx', 'in_idx'])
@pytest.mark.parametrize('which', ['dOut', 'dW'])
@pytest.mark.parametrize('D', DS)
def test_scatter_add_rows_det(D, which, idx):
    """the fixed-order form on random gradients onto a PREFILLED table: bit for bit the order oracle of tests/det_order_ref.py
    (scatter_in_order: ascending source position, added once), as in tests/test_hip_det_order.py. n = 300 with in_idx (segments on both
    sides of the 64-source split when rows repeat), 130 without."""
    n = 300 if idx else N
    g, w0 = _rand(N, D, seed=50 + D), _rand(N, D, seed=51 + D)
    rows = draw_rows(n, 52 + D)
    if idx:
        rows[n // 2:], rows[:7] = np.resize([64, 128, 129, 0], n - n // 2), EDGE_ROWS             # four segments of more than 64 sources
    covers(rows, 'rows')
    ii = draw_rows(n, 53 + D) if idx else None
    want = torch.from_numpy(det_order_ref.scatter_in_order(g.numpy(), ii, rows, w0.numpy()))
    rows_d, ii_d = _i32(rows), None if ii is None else _i32(ii)
    what = f'sbr_scatter_add_rows_det D={D} {which} n={n}'

    def run(make):
        mo, mw = _pick(which, make, 'dOut', 'dW')
        Ob, Wb = mo(N, D, g), mw(N, D, w0)
        call('sbr_scatter_add_rows_det', Ob.ptr, Ob.ld, _p(ii_d), _p(rows_d), Wb.ptr, Wb.ld, n, D, _L().stream())
        unchanged(Ob, g, 'dOut')
        return out(Wb, _named(rows), what=what)

    _assert_bits(both(run, what), want, what + ' against the order oracle')


@pytest.mark.parametrize('which', ['dOut', 'dW'])
@pytest.mark.parametrize('D', DS)
def test_scatter_add_rows_sorted(D, which):
    """rows_sorted / perm: the stable sort of a draw; dOut is two blocks of 65 rows (blk = 65, block_stride = 65 ldo: the second block
    starts past element 2^31 at LD_BIG), perm a draw from its 130 rows. The bound of tests/test_hip_rowops.py::
    test_scatter_add_rows_sorted, (m + 1) u (|dW| + sum|terms|), onto a table prefilled with 0.5."""
    n = 300
    g = _rand(N, D, seed=60 + D)
    src, rows = draw_rows(n, 61 + D), draw_rows(n, 62 + D)
    order = np.argsort(rows, kind='stable')
    perm, rs = covers(src[order], 'perm'), covers(rows[order], 'rows_sorted')
    ref, bound, _ = RR.scatter_add_ref(g, src, rows, N, base=0.5)
    perm_d, rs_d = _i64(perm), _i32(rs)
    what = f'sbr_scatter_add_rows_sorted D={D} {which}'

    def run(make):
        mo, mw = _pick(which, make, 'dOut', 'dW')
        Ob, Wb = mo(N, D, g), mw(N, D, fill=0.5)
        call('sbr_scatter_add_rows_sorted', Ob.ptr, Ob.ld, 65, 65 * Ob.ld, _p(perm_d), _p(rs_d), Wb.ptr, Wb.ld, n, D, _L().stream())
        unchanged(Ob, g, 'dOut')
        return out(Wb, _named(rows), what=what)

    _assert_bound(both(run, what), ref, bound, what)


# ---- sbr_bag_mean_fwd / _bwd ----------------------------------------------------------------------------------------------------------
PAD, T = 4, 4


@functools.lru_cache(maxsize=None)
def bag_world():
    """tags [40 entities, 4] over 130 tag rows: 0, 1, 2 or 4 live tags per entity (1 / cnt is a power of two), a repeated tag, pads in
    the middle; entities 3 and 7 hold the edge rows; the slots' entities are a draw that includes both"""
    rng = np.random.default_rng(404)
    tags = rng.integers(0, N, size=(40, T))
    tags[tags == PAD] = PAD + 1
    for e in range(40):
        if e % 4 == 0:
            tags[e] = PAD
        elif e % 4 == 1:
            tags[e, [0, 1, 3]] = PAD
        elif e % 4 == 2:
            tags[e, [1, 2]] = PAD
    tags[3], tags[7], tags[11] = [0, 63, 64, 65], [127, 128, 129, 129], [64, 128, 129, 0]
    return tags


def _bag_rows(n, seed):
    rows = np.random.default_rng(seed).integers(0, 40, size=n)
    rows[:4] = [3, 7, 11, 0]
    tg = bag_world()[rows]
    covers(tg[tg != PAD], 'the tags of the slots')
    return rows


@pytest.mark.parametrize('idx', [False, True], ids=['no out_idx', 'out_idx'])
@pytest.mark.parametrize('which', ['W', 'out'])
@pytest.mark.parametrize('D', DS)
def test_bag_mean_fwd(D, which, idx):
    """the bound of tests/test_hip_rowops.py::test_bag_mean_fwd_and_bwd: (cnt + 1) u sum|terms| / cnt; all-pad rows are +0"""
    n = 120 if idx else N
    w = _rand(N, D, seed=70 + D)
    rows = _bag_rows(n, 71 + D)
    oi = some_rows(n, 72 + D) if idx else None
    tags_d, rows_d, oi_d = _i32(bag_world()), _i32(rows), None if oi is None else _i32(oi)
    what = f'sbr_bag_mean_fwd D={D} {which}'

    def run(make):
        mw, mo = _pick(which, make, 'W', 'out')
        Wb, Ob = mw(N, D, w), mo(N, D)
        call('sbr_bag_mean_fwd', Wb.ptr, Wb.ld, _p(tags_d), T, PAD, _p(rows_d), Ob.ptr, Ob.ld, _p(oi_d), n, D, _L().stream())
        unchanged(Wb, w, 'W')
        return out(Ob, np.arange(n) if oi is None else oi, what=what)

    got = both(run, what)[torch.as_tensor(np.arange(n) if oi is None else oi)]
    ref, bound, cnt = RR.bag_mean_fwd_ref(w, bag_world(), PAD, rows)
    _assert_bound(got, ref, bound, what)
    assert bool((cnt == 0).any()) and bool((_bits(got[cnt == 0]) == 0).all())


@pytest.mark.parametrize('idx', [False, True], ids=['no in_idx', 'in_idx'])
@pytest.mark.parametrize('which', ['dOut', 'dW'])
@pytest.mark.parametrize('D', DS)
def test_bag_mean_bwd(D, which, idx):
    """float atomics: integer gradient rows, 1 / cnt in {1, 1/2, 1/4}: every term is a multiple of 1/4 and every order of addition gives
    the same bits. The bound of tests/test_hip_rowops.py::test_bag_mean_fwd_and_bwd, (m + 1) u sum|terms|, and equality."""
    n = 300 if idx else N
    g = _ints(N, D, 80 + D)
    rows = _bag_rows(n, 81 + D)
    ii = draw_rows(n, 82 + D) if idx else None
    tags = bag_world()
    ref, bound, m = RR.bag_mean_bwd_ref(g, ii, tags, PAD, rows, N)
    tg = tags[rows]
    live = tg != PAD
    per_slot = g[torch.as_tensor(np.arange(n) if ii is None else ii)].numpy() / np.maximum(live.sum(1), 1)[:, None].astype(np.float32)
    _orders_agree(tg[live], np.repeat(per_slot, live.sum(1), axis=0), N, ref, 'sbr_bag_mean_bwd')
    tags_d, rows_d, ii_d = _i32(tags), _i32(rows), None if ii is None else _i32(ii)
    what = f'sbr_bag_mean_bwd D={D} {which}'

    def run(make):
        mo, mw = _pick(which, make, 'dOut', 'dW')
        Ob, Wb = mo(N, D, g), mw(N, D, fill=0.0)
        call('sbr_bag_mean_bwd', Ob.ptr, Ob.ld, _p(ii_d), _p(tags_d), T, PAD, _p(rows_d), Wb.ptr, Wb.ld, n, D, _L().stream())
        unchanged(Ob, g, 'dOut')
        return out(Wb, _named(tg[live]), what=what)

    got = both(run, what)
    _assert_bound(got, ref, bound, what)
    assert torch.equal(got.double(), ref), what
    assert bool((_bits(got[m[:, 0] == 0]) == 0).all()) and bool((got[PAD] == 0).all())


# ---- sbr_csr_project_fwd / _bwd / _bwd_gather ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def csr_world():
    """40 entities x 130 feature columns: rows of 0 .. 20 entries with values in {-1.5, -1, 0.5, 1, 2}; entity 3 holds the edge
    columns, entity 9 a second copy of 64, 128 and 129; entity 5 is empty"""
    rng = np.random.default_rng(505)
    cols = []
    for e in range(40):
        c = set(rng.choice(N, size=int(rng.integers(0, 21)), replace=False).tolist())
        if e == 3:
            c |= set(EDGE_ROWS)
        if e == 9:
            c |= {64, 128, 129}
        if e == 5:
            c = set()
        cols.append(np.sort(np.fromiter(c, dtype=np.int64, count=len(c))))
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    indices = np.concatenate(cols).astype(np.int32)
    vals = rng.choice(np.array([-1.5, -1.0, 0.5, 1.0, 2.0], dtype=np.float32), size=len(indices))
    return indptr, indices, vals, RR.csr_dense(indptr, indices, vals, 40, N), RR.csr_dense(indptr, indices, None, 40, N)


def _csr_rows(n, seed):
    indptr, indices = csr_world()[:2]
    rows = np.random.default_rng(seed).integers(0, 40, size=n)
    rows[:3] = [3, 9, 5]
    covers(np.concatenate([indices[indptr[r]:indptr[r + 1]] for r in rows]), 'the CSR indices of the slots')
    return rows


@pytest.mark.parametrize('idx', [False, True], ids=['no out_idx', 'out_idx'])
@pytest.mark.parametrize('which', ['Wt', 'out'])
@pytest.mark.parametrize('C', DS)
def test_csr_project_fwd(C, which, idx):
    """Wt [130 feature columns, C] under the CSR indices, out [130, C] under out_idx; C = 5 is the wave-per-row kernel, 64 / 128 the
    workgroup-per-row one. vals given (with out_idx) and NULL (without). The bound of tests/test_hip_rowops.py::
    test_csr_project_branches: (q + 1) u sum|terms|"""
    indptr, indices, vals, dense_v, dense_1 = csr_world()
    n = 120 if idx else N
    wt, b = _rand(N, C, seed=90 + C), _rand(C, seed=91 + C)
    rows = _csr_rows(n, 92 + C)
    oi = some_rows(n, 93 + C) if idx else None
    ops = [_i64(indptr), _i32(indices), torch.from_numpy(vals).to(DEV) if idx else None]
    b_d, rows_d, oi_d = b.to(DEV), _i32(rows), None if oi is None else _i32(oi)
    what = f'sbr_csr_project_fwd C={C} {which}'

    def run(make):
        mw, mo = _pick(which, make, 'Wt', 'out')
        Wb, Ob = mw(N, C, wt), mo(N, C)
        call('sbr_csr_project_fwd', *[_p(o) for o in ops], Wb.ptr, Wb.ld, _p(b_d), _p(rows_d), Ob.ptr, Ob.ld, _p(oi_d), n, C, 0, _L().stream())
        unchanged(Wb, wt, 'Wt')
        return out(Ob, np.arange(n) if oi is None else oi, what=what)

    got = both(run, what)[torch.as_tensor(np.arange(n) if oi is None else oi)]
    ref, bound = RR.csr_project_fwd_ref(dense_v if idx else dense_1, rows, wt, b)
    _assert_bound(got, ref, bound, what)


def _project_bwd_premise(dense, rows, dz, dz_idx, ref, what):
    d = dense[torch.as_tensor(rows)]
    slot, col = np.nonzero(d.numpy())
    z = dz[torch.as_tensor(np.arange(len(rows)) if dz_idx is None else dz_idx)].numpy()
    terms = d.numpy()[slot, col].astype(np.float32)[:, None] * z[slot]
    _orders_agree(col, terms, N, ref, what)


@pytest.mark.parametrize('which', ['dZ', 'dWt'])
@pytest.mark.parametrize('C', DS)
def test_csr_project_bwd(C, which):
    """dWt[col, :] += val * dZ[j, :] with float atomics into a zeroed table: integer dZ and values in {-1.5 .. 2} (multiples of 1/2: every
    order gives the same bits). dZ [130 slots, C] is read by slot (the entry takes no index on it); dWt [130, C] under the CSR indices.
    The bound of tests/test_hip_rowops.py::test_csr_project_branches, (m + 1) u sum|terms|, and equality."""
    indptr, indices, vals, dense_v, _ = csr_world()
    dz = _ints(N, C, 100 + C)
    rows = _csr_rows(N, 101 + C)
    ref, bound = RR.csr_project_bwd_ref(dense_v, rows, dz)
    _project_bwd_premise(dense_v, rows, dz, None, ref, 'sbr_csr_project_bwd')
    ops = [_i64(indptr), _i32(indices), torch.from_numpy(vals).to(DEV)]
    rows_d = _i32(rows)
    named = _named(np.concatenate([indices[indptr[r]:indptr[r + 1]] for r in rows]))
    what = f'sbr_csr_project_bwd C={C} {which}'

    def run(make):
        mz, mw = _pick(which, make, 'dZ', 'dWt')
        Zb, Wb = mz(N, C, dz), mw(N, C, fill=0.0)
        call('sbr_csr_project_bwd', *[_p(o) for o in ops], Zb.ptr, Zb.ld, _p(rows_d), Wb.ptr, Wb.ld, N, C, _L().stream())
        unchanged(Zb, dz, 'dZ')
        return out(Wb, named, what=what)

    got = both(run, what)
    _assert_bound(got, ref, bound, what)
    assert torch.equal(got.double(), ref), what


@pytest.mark.parametrize('idx', [False, True], ids=['no dz_idx', 'dz_idx'])
@pytest.mark.parametrize('which', ['dZ', 'dWt'])
@pytest.mark.parametrize('C', DS4)
def test_csr_project_bwd_gather(C, which, idx):
    """the gather form over the transposed matrix, onto a dWt prefilled with 0.25: dZ [130, C] under dz_idx, dWt [130 feature columns, C]
    (row j = column j; the columns no entity of the batch has keep 0.25 in value). The workspace dZe [40, C] must be dense (lde = C): it
    reaches no crossing. Integer dZ (the entry scatters with float atomics first). The bound of tests/test_hip_rowops.py::
    test_csr_project_branches, (m + 2) u (|dWt| + sum|terms|), and equality."""
    indptr, indices, vals, dense_v, _ = csr_world()
    n = 300 if idx else N
    dz = _ints(N, C, 110 + C)
    rows = _csr_rows(n, 111 + C)
    di = draw_rows(n, 112 + C) if idx else None
    ref, bound = RR.csr_project_bwd_ref(dense_v, rows, dz, di, base=0.25, extra=2)
    _project_bwd_premise(dense_v, rows, dz, di, ref - 0.25, 'sbr_csr_project_bwd_gather')
    mt = sp.csr_matrix((vals, indices, indptr), shape=(40, N)).T.tocsr()
    mt.sort_indices()
    ops = [_i64(mt.indptr), _i32(mt.indices), torch.from_numpy(mt.data.astype(np.float32)).to(DEV)]
    rows_d, di_d = _i32(rows), None if di is None else _i32(di)
    what = f'sbr_csr_project_bwd_gather C={C} {which}'

    def run(make):
        mz, mw = _pick(which, make, 'dZ', 'dWt')
        Zb, Wb, Eb = mz(N, C, dz), mw(N, C, fill=0.25), compact(40, C)
        call('sbr_csr_project_bwd_gather', *[_p(o) for o in ops], Zb.ptr, Zb.ld, _p(di_d), _p(rows_d), n, Eb.ptr, C, 40, Wb.ptr, Wb.ld, N, C,
             _L().stream())
        unchanged(Zb, dz, 'dZ')
        out(Eb, what='the workspace dZe')
        return out(Wb, np.flatnonzero(np.diff(mt.indptr) > 0), what=what)               # a column no entity has is not written at all

    got = both(run, what)
    _assert_bound(got, ref, bound, what)
    assert torch.equal(got.double(), ref), what


# ---- the score matrix: sbr_floor_scores, sbr_uniform_rows_f32 ------------------------------------------------------------------------------
@pytest.mark.parametrize('n_cols', [5, 200])
def test_floor_scores(n_cols):
    """x[x < mu] = mu in place on [130, n_cols], NaN and +-inf among the values; rows 64 and 128 hold values on both sides of mu.
    evalk_ref.floor_ref, bit for bit; the columns behind n_cols are guard band"""
    mu = 0.1
    x = _rand(N, n_cols, seed=n_cols)
    x[64, 0], x[64, 1], x[128, 0], x[128, 1], x[129, 2] = -1.0, 1.0, mu - 1e-3, mu + 1e-3, float('nan')
    x[3, 4], x[65, 3] = -float('inf'), float('inf')
    assert all(bool((x[r] < mu).any()) and bool((x[r] > mu).any()) for r in (64, 128))

    def run(make):
        b = make(N, n_cols, x)
        call('sbr_floor_scores', b.ptr, N, n_cols, b.ld, mu, _L().stream())
        return out(b, what='sbr_floor_scores')

    _assert_bits(both(run, f'sbr_floor_scores n_cols={n_cols}'), E.floor_ref(x, mu), 'sbr_floor_scores')


@pytest.mark.parametrize('n_items', [5, 200])
def test_uniform_rows(n_items):
    """out [Bu = 130, n_items] with u_idx a permutation of user ids spread past 2^31: the Philox restatement of tests/naive_ref.py, bit for
    bit (n_items = 5: a ragged last block of four)"""
    ids = (perm_rows(n_items) * 33_554_467).astype(np.int64)
    ids_d = _i64(ids)
    seed = 0x9E3779B97F4A7C15

    def run(make):
        b = make(N, n_items)
        call('sbr_uniform_rows_f32', seed, _p(ids_d), N, n_items, b.ptr, b.ld, _L().stream())
        return out(b, what='sbr_uniform_rows_f32')

    got = both(run, f'sbr_uniform_rows_f32 n_items={n_items}')
    assert np.array_equal(got.numpy().view(np.int32), naive_ref.uniform_rows_ref(seed, ids, n_items).view(np.int32))
