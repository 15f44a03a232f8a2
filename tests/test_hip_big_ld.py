"""Address arithmetic past 2^31 and 2^32 elements in the entries that take a leading dimension: the fit-matrix kernels and the
full-catalogue evaluation kernels form ``row * ld + col``, and an ``int`` row or an unsigned product there would corrupt a resident
items x items matrix silently at 46,341 items (2^31 elements) or 65,536 (2^32). No large operand is built: one operand of each call is a
view of at most 130 rows with row stride LD_BIG = 2^25 + 64 into one untouched 16.1 GiB buffer (hip_testutil._BigLd), so that row 64
starts past element 2^31 (a signed 32-bit product wraps there), row 128 past element 2^32 (an unsigned one), and every row from 32 on
past byte 2^32; everything else is compact. Every operand that has a leading dimension gets LD_BIG in a case of its own.

Each case asserts (a) the entry's existing independent reference under the bound its own test module uses (tests/*_ref.py; nothing new),
(b) bit equality with the same call at ld = 192 — a multiple of 64 like LD_BIG, so alignment and vector-width branches agree; 256 where
a row is wider than 192 — and (c) the guard bands of the view and, for row-range entries, the full width of the rows outside the range.
No entry refuses LD_BIG, and no entry's summation order depends on ld, so (b) holds everywhere.

Entries whose operand admits at most 128 rows (the f x f, b x b and n x n matrices of the block kernels: G of the Gram entries, W of
sbr_rotate_cols_f32, T of sbr_tri_solve_rows_f32, Ltop / Utop, sbr_chol_f32, sbr_sym_eig_f32) cross element 2^31 and byte 2^32 only;
their docstrings say so."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import als_ref
import block_ref as B
import ease_ref
import evalk_ref as E
import ifknn_ref
import knn_ref
import p3alpha_ref
import rbmf_ref
import slim_ref
import svd_ref
from hip_testutil import DEV, LD_BIG, S, U32, _BigLd, _Buf, _assert_bits, _assert_bound, _bits, _i32, _i64, _L, _p, call

pytestmark = pytest.mark.gpu

LD_SMALL = 192
N = 130
RANGES = (None, (60, 70), (126, 130))


@pytest.fixture(scope='module', autouse=True)
def big_buffer():
    """the one large allocation of the module (skips the module when the device has no room for it), freed at the end"""
    _BigLd._flat()
    torch.cuda.reset_peak_memory_stats()
    yield
    print(f'peak device memory of the module: {torch.cuda.max_memory_allocated()} bytes')
    _BigLd.release()


def _big(rows, cols, data=None):
    return _BigLd(rows, cols, data=None if data is None else _t(data))


def _small(rows, cols, data=None):
    return _Buf(rows, cols, ld=LD_SMALL if cols <= LD_SMALL else 256, data=None if data is None else _t(data))


def _compact(rows, cols, data=None):
    return _Buf(rows, cols, data=None if data is None else _t(data))


BOTH = ((_big, 'ld = LD_BIG'), (_small, 'ld = 192'))


def _t(a):
    return a if isinstance(a, torch.Tensor) else B.as_torch(a)


def _unchanged(buf, data, what):
    """an input: what surrounds the view holds its NaN pattern, and the view holds the bits it was given"""
    _assert_bits(buf.check_untouched(what=what).contiguous(), _t(data).reshape(buf.rows, buf.cols), f'{what} was written')


def _out(buf, rows=None, what=''):
    return buf.check_untouched(rows, what=what).contiguous()


def _both(run, what):
    """run(make) -> a tensor or a tuple of tensors, once per layout; the LD_BIG result, after checking that the two agree in bits"""
    got = [run(make) for make, _ in BOTH]
    for a, b in zip(*[g if isinstance(g, tuple) else (g,) for g in got]):
        a, b = (v if v.dtype == torch.float32 else v.to(torch.int32).view(torch.float32) for v in (a, b))
        _assert_bits(a, b, f'{what}: {BOTH[0][1]} against {BOTH[1][1]}')
    return got[0]


def _ws(nbytes):
    return torch.empty(max(nbytes // 4, 1), device=DEV)


def _info():
    return torch.zeros(1, device=DEV, dtype=torch.int32)


def _rows_mask(rng_):
    m = torch.zeros(N, dtype=torch.bool)
    m[slice(None) if rng_ is None else slice(*rng_)] = True
    return m


def test_the_view_reaches_both_crossings():
    buf = _BigLd(N, 8)
    assert all(buf.crossings.values()) and 64 * LD_BIG >= 1 << 31 and 128 * LD_BIG >= 1 << 32 and 4 * 32 * LD_BIG >= 1 << 32
    assert 63 * LD_BIG < 1 << 31 and 127 * LD_BIG < 1 << 32 and LD_BIG % 64 == 0 and LD_SMALL % 64 == 0
    assert _BigLd(128, 8).crossings == {'2^31 elements': True, '2^32 elements': False, '2^32 bytes': True}
    assert buf.t[128].data_ptr() - buf.t.data_ptr() == 4 * 128 * LD_BIG
    buf.t[128, 3] = 5.0                                      # the helper itself: a write into an unaddressed row is noticed
    with pytest.raises(AssertionError, match='outside the addressed'):
        buf.check_untouched(slice(0, 128))
    buf.t[128, 3] = float('nan')
    buf.bands[2][63, 0] = 1.0                                # and one into the band in front of row 64
    with pytest.raises(AssertionError, match='guard elements'):
        buf.check_untouched()


# ---- evaluation -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def eval_world():
    """scores [130 users, 200 items] with exact ties in rows 64 (seven values) and 128 (one value), and an exclusion CSR over 130 users
    in which user 5 has no entry and users 63, 64, 65, 127, 128, 129 have some"""
    rng = np.random.default_rng(130200)
    scores = rng.standard_normal((N, 200)).astype(np.float32)
    scores[64] = (np.arange(200) % 7).astype(np.float32)
    scores[128] = 0.5
    lists = [np.sort(rng.choice(200, size=int(rng.integers(1, 25)), replace=False)) for _ in range(N)]
    lists[5] = np.zeros(0, dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int64)
    indices = np.concatenate(lists).astype(np.int32)
    assert all(len(lists[u]) > 0 for u in (63, 64, 65, 127, 128, 129))
    return torch.from_numpy(scores), (indptr, indices), rng.permutation(N).astype(np.int64)


@pytest.mark.parametrize('permuted', [False, True])
def test_mask_scores_and_the_shard_form(permuted):
    scores, csr, perm = eval_world()
    u = perm if permuted else None
    indptr, indices, u_d = _i64(csr[0]), _i32(csr[1]), None if u is None else _i64(u)

    def whole(make):
        b = make(N, 200, scores)
        call('sbr_mask_scores', b.ptr, b.ld, _p(u_d), _p(indptr), _p(indices), N, _L().stream())
        return _out(b, what='sbr_mask_scores')

    _assert_bits(_both(whole, 'sbr_mask_scores'), E.mask_ref(scores, u, csr), 'sbr_mask_scores')
    off, n = 37, 150
    part = scores[:, off:off + n].contiguous()

    def shard(make):
        b = make(N, n, part)
        call('sbr_mask_scores_shard', b.ptr, b.ld, _p(u_d), _p(indptr), _p(indices), N, off, n, _L().stream())
        return _out(b, what='sbr_mask_scores_shard')

    _assert_bits(_both(shard, 'sbr_mask_scores_shard'), E.mask_ref(part, u, csr, item_offset=off), 'sbr_mask_scores_shard')


@pytest.mark.parametrize('k', [10, 128])
def test_topk_rows(k):
    scores = eval_world()[0]

    def run(make):
        sb, v, x = make(N, 200, scores), _compact(N, k), _compact(N, k)
        call('sbr_topk_rows', sb.ptr, sb.ld, N, 200, k, v.ptr, x.ptr, _L().stream())
        _unchanged(sb, scores, 'scores')
        return _out(v, what='values'), _bits(_out(x, what='indices'))

    val, idx = _both(run, f'sbr_topk_rows k={k}')
    want = E.topk_ref(scores, k)
    bad = [r for r in range(N) if not E.same_lists((val[r:r + 1], idx[r:r + 1]), (want[0][r:r + 1], want[1][r:r + 1]))]
    assert not bad, f'rows {bad} differ from the stable descending order'
    assert idx[128].tolist() == list(range(k))               # the all-tied row: ascending index


def test_csr_rows_to_dense():
    rng = np.random.default_rng(7)
    d = (rng.random((150, 200)) < 0.1) * rng.uniform(0.5, 2.0, size=(150, 200))
    d[11] = 0
    x = sp.csr_matrix(d.astype(np.float32))
    x.sort_indices()
    ent = rng.integers(0, 150, size=N).astype(np.int64)      # unsorted, with repeats
    ent[[64, 128]], ent[[3, 65]], ent[[20, 129]] = 149, 11, -1
    ref = np.where(ent[:, None] >= 0, np.asarray(x.todense(), dtype=np.float32)[np.maximum(ent, 0)], np.float32(0))
    ops = [_i64(x.indptr), _i32(x.indices), torch.from_numpy(x.data).to(DEV), _i64(ent)]

    def run(make):
        out = make(N, 200)
        call('sbr_csr_rows_to_dense', *[_p(o) for o in ops], N, 200, out.ptr, out.ld, _L().stream())
        return _out(out, what='sbr_csr_rows_to_dense')

    _assert_bits(_both(run, 'sbr_csr_rows_to_dense'), torch.from_numpy(ref), 'sbr_csr_rows_to_dense')
    assert len(set(ent.tolist())) < N and list(ent) != sorted(ent)


# ---- sparse products and walks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tile_cols', [64, 0])
def test_csr_rows_times_csr(tile_cols):
    x, rows7, y = knn_ref.ordered_product_operands(134)
    rows = np.resize(rows7, N)
    ref = knn_ref.csr_rows_times_csr_ordered(x, rows, y)
    ops = [_i64(x.indptr), _i32(x.indices), torch.from_numpy(x.data).to(DEV), _i64(rows)]
    yo = [_i64(y.indptr), _i32(y.indices), torch.from_numpy(y.data).to(DEV)]

    def run(make):
        out = make(N, 134)
        call('sbr_csr_rows_times_csr', *[_p(o) for o in ops], N, *[_p(o) for o in yo], 134, tile_cols, out.ptr, out.ld, _L().stream())
        return _out(out, what='sbr_csr_rows_times_csr')

    _assert_bits(_both(run, f'sbr_csr_rows_times_csr tile_cols={tile_cols}'), torch.from_numpy(ref), 'the order oracle')


def _csr_ops(x):
    xt = sp.csr_matrix(x.T)
    xt.sort_indices()
    return [_i64(x.indptr), _i32(x.indices), _i64(xt.indptr), _i32(xt.indices)]


@functools.lru_cache(maxsize=None)
def gram_world():
    """the '97x130' world of tests/test_hip_ease.py: density 0.1, an empty column (17) and an empty row (40)"""
    d = np.random.default_rng(97 + 130).random((97, 130)) < 0.1
    d[:, 17] = False
    d[40] = False
    x = sp.csr_matrix(d.astype(np.float64))
    x.sort_indices()
    return x


@pytest.mark.parametrize('rows', RANGES)
@pytest.mark.parametrize('tile_cols', [0, 64])
def test_gram_dense(rows, tile_cols):
    x = gram_world()
    ref = torch.from_numpy((np.asarray((x.T @ x).todense()) + 3. * np.eye(N)).astype(np.float32))      # integers: exact
    r0, r1 = rows or (0, N)
    ops = _csr_ops(x)

    def run(make):
        out = make(N, N)
        call('sbr_gram_dense', *[_p(o) for o in ops], 97, N, r0, r1, 3., tile_cols, out.ptr, out.ld, _L().stream())
        return _out(out, _rows_mask(rows), what=f'sbr_gram_dense rows {rows}')

    got = _both(run, f'sbr_gram_dense rows {rows}')
    _assert_bits(got[r0:r1], ref[r0:r1], f'sbr_gram_dense rows {rows}')
    assert bool(torch.isnan(got[:r0]).all()) and bool(torch.isnan(got[r1:]).all())


@functools.lru_cache(maxsize=None)
def p3_world():
    x = p3alpha_ref.world('97x130')
    return x, p3alpha_ref.walk32(x)


@pytest.mark.parametrize('rows', RANGES)
def test_p3_walk_dense(rows):
    x, w = p3_world()
    r0, r1 = rows or (0, N)
    ops = _csr_ops(x)

    def run(make):
        out = make(N, N)
        call('sbr_p3_walk_dense', *[_p(o) for o in ops], 97, N, r0, r1, 64, out.ptr, out.ld, _L().stream())
        return _out(out, _rows_mask(rows), what=f'sbr_p3_walk_dense rows {rows}')

    got = _both(run, f'sbr_p3_walk_dense rows {rows}')
    _assert_bits(got[r0:r1], torch.from_numpy(w)[r0:r1], f'sbr_p3_walk_dense rows {rows}')
    assert bool(torch.isnan(got[:r0]).all()) and bool(torch.isnan(got[r1:]).all())


@pytest.mark.parametrize('which', ['W', 'out'])
def test_p3_score_rows(which):
    """alpha = 1: bit for bit against the order oracle. W [130, 130] or out [130 picked users, 130] at LD_BIG"""
    x, w = p3_world()
    rows = np.random.default_rng(3).integers(0, 97, size=N).astype(np.int64)
    rows[[64, 128]] = 95, 3                                   # the empty user and the user holding every item
    ref = p3alpha_ref.pre_power32(x, w, rows)
    ops = [_i64(x.indptr), _i32(x.indices), _i64(rows)]

    def run(make):
        wb = (make if which == 'W' else _compact)(N, N, w)
        out = (make if which == 'out' else _compact)(N, N)
        call('sbr_p3_score_rows', *[_p(o) for o in ops], N, wb.ptr, wb.ld, N, 1.0, out.ptr, out.ld, _L().stream())
        _unchanged(wb, w, 'W')
        return _out(out, what='out')

    _assert_bits(_both(run, f'sbr_p3_score_rows {which}'), torch.from_numpy(ref), 'the order oracle')


# ---- dense-block kernels ----------------------------------------------------------------------------------------------------------------
def test_ease_weights():
    P = B.ease_inputs(N)

    def run(make):
        pb, db = make(N, N, P), _compact(1, N)
        call('sbr_ease_weights_f32', pb.ptr, N, pb.ld, db.ptr, _L().stream())
        B.same_bits(_out(db, what='diag').numpy()[0], np.ascontiguousarray(np.diagonal(P)), 'diag scratch')
        return _out(pb, what='P')

    B.check_ease(_both(run, 'sbr_ease_weights_f32').numpy(), P)


def test_spd_inverse():
    """n = 130: three pivot blocks, the last one (rows 128, 129) past element 2^32; the bound of tests/test_hip_ease.py::test_spd_inverse"""
    a = ease_ref.random_spd(N, 1, seed=1000 + 2 * N + 1)
    inv, e = np.linalg.inv(a), ease_ref.e_ref(a)
    need = int(_L().lib().sbr_spd_inverse_f32_workspace(N))

    def run(make):
        ab, ws, info = make(N, N, a.astype(np.float32)), _ws(need), _info()
        call('sbr_spd_inverse_f32', ab.ptr, N, ab.ld, _p(ws), need, _p(info), _L().stream())
        assert int(info.item()) == 0
        return _out(ab, what='A')

    g = _both(run, 'sbr_spd_inverse_f32').double().numpy()
    err, asym = np.abs(g - inv).max(), np.abs(g - g.T).max()
    print(f'spd_inverse n={N} at LD_BIG: e_ref {e:.3e} kernel err {err:.3e} ratio {err / e:.3f} asymmetry {asym:.3e}')
    assert err <= ease_ref.FACTOR * e and asym <= ease_ref.FACTOR * e


SLIM_SWEEPS = 30


@functools.lru_cache(maxsize=None)
def slim_case():
    x = slim_ref.world(90, N, 0.1, seed=90 + N)
    g = slim_ref.gram(x)
    l1, l2 = slim_ref.penalties(90, 0.01, 0.5)
    return (np.asarray(g, dtype=np.float32), l1, l2) + slim_ref.e_ref(g, l1, l2, SLIM_SWEEPS, None)


@pytest.mark.parametrize('which', ['G', 'W'])
def test_slim_cd(which):
    """the yardstick rule of tests/test_hip_slim.py: error against the float64 restatement <= 8 x that of the float32 restatement"""
    g, l1, l2, e, w64, _ = slim_case()

    def run(make):
        gb = (make if which == 'G' else _compact)(N, N, g)
        wb = (make if which == 'W' else _compact)(N, N)
        n_iter = torch.full((N,), -77, device=DEV, dtype=torch.int32)
        call('sbr_slim_cd_f32', gb.ptr, N, gb.ld, 0, N, float(l1), float(l2), SLIM_SWEEPS, 0., wb.ptr, wb.ld, _p(n_iter), _L().stream())
        _unchanged(gb, g, 'G')
        return _out(wb, what='W'), n_iter.cpu()

    w, n_iter = _both(run, f'sbr_slim_cd_f32 {which}')
    err = float(np.abs(w.double().numpy() - w64).max())
    print(f'slim 90x{N} {which} at LD_BIG: e_ref {e:.3e} kernel err {err:.3e} ratio {err / e if e else 0.:.3f}')
    assert err <= slim_ref.FACTOR * e
    assert bool((w >= 0).all()) and not bool(w.diagonal().any()) and bool((n_iter != -77).all())


def test_row_norms_and_dense_knn_topk():
    """integer features (exact dots): norms, lists, values and lengths bit for bit against the float32 restatement of ifknn_ref"""
    n, d, k, shrinkage = N, 33, 5, 2.5
    rng = np.random.default_rng(100 * n + d)
    f = rng.integers(0, 5, (n, d)).astype(np.float32)
    f[n - 1], f[n // 2], f[n // 3] = -f[0], 0, f[1]
    want = ifknn_ref.lists_f32_exact(f, k, shrinkage)
    norms_ref = np.sqrt((f.astype(np.float64) ** 2).sum(axis=1).astype(np.float32))

    def run(make):
        fb, norms = make(n, d, f), _compact(n, 1)
        call('sbr_row_norms_f32', fb.ptr, n, d, fb.ld, norms.ptr, _L().stream())
        idx, val, length = _compact(n, k), _compact(n, k), _compact(n, 1)
        call('sbr_dense_knn_topk', fb.ptr, norms.ptr, n, d, fb.ld, 0, n, shrinkage, k, idx.ptr, val.ptr, length.ptr, _L().stream())
        _unchanged(fb, f, 'F')
        return _out(norms, what='norms')[:, 0], _bits(_out(idx, what='nbr_idx')), _out(val, what='nbr_val'), _bits(_out(length, what='nbr_len'))[:, 0]

    norms, idx, val, length = _both(run, 'sbr_row_norms_f32 / sbr_dense_knn_topk')
    B.same_bits(norms.numpy(), norms_ref, 'norms')
    assert np.array_equal(idx.numpy(), want[0]) and np.array_equal(length.numpy(), want[2])
    B.same_bits(val.numpy(), want[1], 'nbr_val')


@pytest.mark.parametrize('entry,reg', [('sbr_gram_f32', ()), ('sbr_als_gram_f32', (B.GRAM_REG,))])
@pytest.mark.parametrize('which,f', [('Y', 7), ('Y', 128), ('G', 128)])
def test_gram_entries(entry, reg, which, f):
    """Y [130, f] at LD_BIG crosses both; G [f, f] admits 128 rows: its last row starts past element 2^31 and byte 2^32, not past
    element 2^32. Integer inputs: bit for bit against integer arithmetic (block_ref.check_gram_exact)"""
    Y = B.gram_inputs(N, f, 'int')
    need = int(_L().lib().sbr_als_gram_f32_workspace(N, f))

    def run(make):
        yb = (make if which == 'Y' else _compact)(N, f, Y)
        gb = (make if which == 'G' else _compact)(f, f)
        call(entry, yb.ptr, N, yb.ld, f, *reg, gb.ptr, gb.ld, _p(_ws(need)), need, _L().stream())
        _unchanged(yb, Y, 'Y')
        return _out(gb, what='G')

    B.check_gram_exact(_both(run, f'{entry} {which}').numpy(), Y, *reg)


@functools.lru_cache(maxsize=None)
def als_case():
    f, alpha = 65, 40.
    x = als_ref.world(N, N, 0.1, seed=2 * N + f)
    y = als_ref.uniform_factors(N, f, seed=7 * f)
    g = als_ref.gram32(y, 0.01)
    ref = als_ref.half_sweep32(x, y, alpha, g)
    return x, y, g, alpha, als_ref.backward_error(x, y, g, alpha, ref)


@pytest.mark.parametrize('which', ['Y', 'X'])
def test_als_solve_rows(which):
    """130 users x 130 items, f = 65: the backward-error rule of tests/test_hip_als.py::test_half_sweep (<= 8 x the yardstick's)"""
    x, y, g, alpha, be_ref = als_case()
    f = y.shape[1]
    ops = [_i64(x.indptr), _i32(x.indices), None]
    gd = torch.from_numpy(g).to(DEV).contiguous()

    def run(make):
        yb = (make if which == 'Y' else _compact)(N, f, y)
        out, info = (make if which == 'X' else _compact)(N, f), _info()
        call('sbr_als_solve_rows_f32', *[_p(o) for o in ops], 0, N, yb.ptr, N, yb.ld, f, _p(gd), alpha, out.ptr, out.ld, _p(info), _L().stream())
        assert int(info.item()) == 0
        _unchanged(yb, y, 'Y')
        return _out(out, what='X')

    got = _both(run, f'sbr_als_solve_rows_f32 {which}')
    be = als_ref.backward_error(x, y, g, alpha, got.numpy())
    print(f'als solve {N}x{N} f={f} {which} at LD_BIG: backward error {be:.3e} yardstick {be_ref:.3e} ratio {be / be_ref:.3f}')
    assert be <= als_ref.BACKWARD_FACTOR * be_ref and bool(torch.isfinite(got).all())
    assert not bool(_bits(got[1]).any())                       # the empty row: +0.0


@pytest.mark.parametrize('which,n,m', [('out', N, 90), ('D', 90, N)])
def test_csr_times_dense(which, n, m):
    """out [130, 65] or D [130, 65] at LD_BIG; the bound of tests/test_hip_svd.py::test_csr_times_dense (nnz u |X| |D|)"""
    c = 65
    rng = np.random.default_rng(n + c)
    d = (rng.random((n, m)) < 0.15).astype(np.float64)
    d[1], d[2], d[3] = 0, 0, 1
    d[2, m // 2] = 1
    d *= rng.uniform(-2, 2, size=d.shape)
    x = svd_ref.canonical(sp.csr_matrix(d))
    D = np.random.default_rng(c).standard_normal((m, c)).astype(np.float32)
    ops = [_i64(x.indptr), _i32(x.indices), torch.from_numpy(x.data.astype(np.float32)).to(DEV)]

    def run(make):
        db = (make if which == 'D' else _compact)(m, c, D)
        out = (make if which == 'out' else _compact)(n, c)
        call('sbr_csr_times_dense_f32', *[_p(o) for o in ops], 0, n, db.ptr, m, db.ld, c, out.ptr, out.ld, _L().stream())
        _unchanged(db, D, 'D')
        return _out(out, what='out')

    got = _both(run, f'sbr_csr_times_dense_f32 {which}')
    x32 = np.asarray(x.astype(np.float32).todense(), dtype=np.float64)
    nnz = torch.from_numpy(np.diff(x.indptr).astype(np.float64))[:, None]
    _assert_bound(got, torch.from_numpy(x32 @ D.astype(np.float64)), nnz * U32 * torch.from_numpy(np.abs(x32) @ np.abs(D.astype(np.float64))), 'csr x dense')
    assert not bool(_bits(got[1]).any())


@pytest.mark.parametrize('which,b', [('Y', 65), ('out', 65), ('in place', 65), ('W', 128)])
def test_rotate_cols(which, b):
    """Y, out [130, b] cross both; W [b, b] admits 128 rows: past element 2^31 and byte 2^32 only. block_ref.check_rotate_float"""
    Y, W, lam = B.rotate_float_inputs(N, b)

    def run(make):
        yb = (make if which in ('Y', 'in place') else _compact)(N, b, Y)
        wb = (make if which == 'W' else _compact)(b, b, W)
        ob = yb if which == 'in place' else (make if which == 'out' else _compact)(N, b)
        lb, sb = _compact(1, b, lam[None, :]), _compact(1, b)
        call('sbr_rotate_cols_f32', yb.ptr, N, yb.ld, b, wb.ptr, wb.ld, lb.ptr, sb.ptr, ob.ptr, ob.ld, _L().stream())
        _unchanged(wb, W, 'W')
        if which != 'in place':
            _unchanged(yb, Y, 'Y')
        return _out(ob, what='out'), _out(sb, what='s')[0]

    out, s = _both(run, f'sbr_rotate_cols_f32 {which}')
    B.check_rotate_float(out.numpy(), s.numpy(), Y, W, lam)


@pytest.mark.parametrize('which', ['Y', 'U'])
def test_col_residual(which):
    f = 65
    Y, Um, s, _ = B.col_residual_inputs(N, f, 'float')
    need = int(_L().lib().sbr_col_residual_f32_workspace(N, f))

    def run(make):
        yb = (make if which == 'Y' else _compact)(N, f, Y)
        ub = (make if which == 'U' else _compact)(N, f, Um)
        sb, rb = _compact(1, f, s[None, :]), _compact(1, f)
        call('sbr_col_residual_f32', yb.ptr, yb.ld, ub.ptr, ub.ld, sb.ptr, N, f, rb.ptr, _p(_ws(need)), need, _L().stream())
        _unchanged(yb, Y, 'Y')
        _unchanged(ub, Um, 'U')
        return _out(rb, what='res')[0]

    B.check_col_residual_float(_both(run, f'sbr_col_residual_f32 {which}').numpy(), Y, Um, s)


@pytest.mark.parametrize('which,r', [('in place', 65), ('in place', 127), ('T', 127)])
def test_tri_solve_rows(which, r):
    """130 rows in place (ldi = ldo = LD_BIG) cross both; T [r, r] at LD_BIG, r = 127: past element 2^31 and byte 2^32 only.
    block_ref.check_tri: |x T - b| <= gamma_r |x| |T|"""
    T = B.tri_inputs(r)[1]
    b = np.random.default_rng(80 + r).standard_normal((N, r)).astype(np.float32)
    for upper in (0, 1):
        for unit in (0, 1):
            def run(make):
                xb = (make if which == 'in place' else _compact)(N, r, b)
                tb = (make if which == 'T' else _compact)(r, r, T)
                call('sbr_tri_solve_rows_f32', xb.ptr, xb.ld, N, r, tb.ptr, tb.ld, upper, unit, xb.ptr, xb.ld, _L().stream())
                _unchanged(tb, T, 'T')
                return _out(xb, what='in place')

            B.check_tri(_both(run, f'sbr_tri_solve_rows_f32 {which} r={r}').numpy(), b, T, upper, unit)


def _lu_chain(ab, r, lb, ub, slab):
    n = ab.rows
    need = int(_L().lib().sbr_maxvol_f32_workspace(n, slab))
    ws, idx, info = torch.zeros(need // 4, device=DEV, dtype=torch.int32), torch.zeros(r, device=DEV, dtype=torch.int32), _info()
    for k in range(r):
        call('sbr_maxvol_lu_step_f32', ab.ptr, n, ab.ld, r, k, _p(idx), lb.ptr, lb.ld, ub.ptr, ub.ld, _p(info), _p(ws), need, slab, _L().stream())
    assert int(info.item()) == 0
    return idx


@pytest.mark.parametrize('which,r', [('A', 7), ('A', 65), ('Ltop', 65), ('Utop', 65)])
def test_maxvol_lu_chain(which, r):
    """A [130, r] at LD_BIG crosses both; Ltop / Utop [65, 65]: row 64 alone lies past element 2^31. The checks of
    tests/test_hip_rbmf.py::test_lu_chain: the oracle's pivot order, |L U - A| <= gamma_r |L| |U|, Ltop = L[idx] bit for bit"""
    u, idx64, _, _, _, ratio = rbmf_ref.lu_input(N, r)
    assert ratio <= rbmf_ref.RATIO_MAX

    def run(make):
        ab = (make if which == 'A' else _compact)(N, r, u)
        lb = (make if which == 'Ltop' else _compact)(r, r)
        ub = (make if which == 'Utop' else _compact)(r, r)
        idx = _lu_chain(ab, r, lb, ub, 64)
        return _out(ab, what='A'), _out(lb, what='Ltop'), _out(ub, what='Utop'), idx.cpu()

    L32, ltop, utop, idx = _both(run, f'sbr_maxvol_lu_step_f32 {which} r={r}')
    L, ut, idx = L32.double().numpy(), utop.double().numpy(), idx.numpy()
    assert np.array_equal(idx, idx64)
    assert bool((np.abs(L @ ut - u.astype(np.float64)) <= rbmf_ref.gamma(r) * (np.abs(L) @ np.abs(ut))).all())
    assert np.array_equal(ltop.numpy(), L32.numpy()[idx]) and not np.triu(ltop.numpy(), 1).any() and not np.tril(ut, -1).any()


@pytest.mark.parametrize('r', [7, 65])
def test_maxvol_swap_chain(r):
    """B = U inv(U[idx]) [130, r] at LD_BIG from the LU start (compact launches), then raw swap launches on it until eight in a row
    change nothing. The checks of tests/test_hip_rbmf.py::test_maxvol_from_the_lu_start_and_the_idle_launches"""
    ops = S().ops
    u = rbmf_ref.lu_input(N, r)[0]
    i64, s64, ratio = rbmf_ref.maxvol(u)
    i32 = rbmf_ref.maxvol(u, dtype=np.float32)[0]
    start = torch.from_numpy(u).to(DEV)
    idx0, ltop, _ = ops.maxvol_lu(start, 64)
    ops.tri_solve_rows(start, ltop, unit=True, out=start)
    need = int(_L().lib().sbr_maxvol_f32_workspace(N, 64))

    def run(make):
        bb = make(N, r, start.cpu())
        ws, idx, counter = torch.zeros(need // 4, device=DEV, dtype=torch.int32), idx0.to(torch.int32).clone(), _info()
        step = 0
        while True:
            before = int(counter.item())
            for _ in range(8):
                call('sbr_maxvol_swap_step_f32', bb.ptr, N, bb.ld, r, rbmf_ref.TOL, step, _p(idx), _p(counter), _p(ws), need, 64, _L().stream())
                step += 1
            if int(counter.item()) == before:
                break
            assert step < 8 * 64
        return _out(bb, what='B'), idx.cpu(), counter.cpu()

    _, idx, swaps = _both(run, f'sbr_maxvol_swap_step_f32 r={r}')
    cert = rbmf_ref.certificate(u, idx.numpy())
    print(f'maxvol r={r} n={N} at LD_BIG: {int(swaps)} swaps (float64 {s64}), ratio {ratio:.5f}, certificate {cert:.7f}')
    assert cert <= rbmf_ref.TOL + rbmf_ref.slack(u, i32, r)
    if ratio <= rbmf_ref.RATIO_MAX:
        assert set(idx.tolist()) == set(i64.tolist()) and int(swaps) == s64


@pytest.mark.parametrize('which', ['K', 'R'])
def test_cholesky(which):
    """n = 128, the largest the entry admits: row 127 starts past element 2^31 and byte 2^32, not past element 2^32"""
    n = 128
    K = B.chol_input(n)
    low = np.tril(K)

    def run(make):
        kb, rb, info = (make if which == 'K' else _compact)(n, n, low), (make if which == 'R' else _compact)(n, n), _info()
        call('sbr_chol_f32', kb.ptr, n, kb.ld, rb.ptr, rb.ld, _p(info), _L().stream())
        assert int(info.item()) == 0
        _unchanged(kb, low, 'K')
        return _out(rb, what='R')

    B.check_chol(_both(run, f'sbr_chol_f32 {which}').numpy(), K)


@pytest.mark.parametrize('which', ['A', 'W'])
def test_sym_eig(which):
    """n = 128, the largest the entry admits: past element 2^31 and byte 2^32 only. The rule of tests/test_hip_svd.py::test_sym_eig:
    residual and orthogonality <= 8 x those of LAPACK's float32 eigh on the same matrix"""
    n = 128
    a = svd_ref.eig_inputs(n)['gram']
    need = int(_L().lib().sbr_sym_eig_f32_workspace(n))

    def run(make):
        ab, wb, lb = (make if which == 'A' else _compact)(n, n, a), (make if which == 'W' else _compact)(n, n), _compact(1, n)
        ws, info = torch.empty(need // 8, device=DEV, dtype=torch.float64), _info()
        call('sbr_sym_eig_f32', ab.ptr, n, ab.ld, wb.ptr, wb.ld, lb.ptr, _p(info), _p(ws), need, _L().stream())
        assert int(info.item()) == 0
        _unchanged(ab, a, 'A')
        return _out(lb, what='lam')[0], _out(wb, what='W')

    lam, w = (v.numpy() for v in _both(run, f'sbr_sym_eig_f32 {which}'))
    (res, orth), (res32, orth32) = svd_ref.eig_figures(a, lam, w), svd_ref.eig_figures(a, *svd_ref.eigh32(a))
    print(f'sym_eig n={n} {which} at LD_BIG: residual {res:.3e} (LAPACK {res32:.3e}), orthogonality {orth:.3e} (LAPACK {orth32:.3e})')
    assert res32 > 0 and orth32 > 0 and res <= svd_ref.EIG_FACTOR * res32 and orth <= svd_ref.EIG_FACTOR * orth32
    assert bool((np.diff(lam) <= 0).all()) and bool((w[np.abs(w).argmax(axis=0), np.arange(n)] > 0).all())
