"""GPU: the evaluation kernels of csrc/topk.hip (sbr_mask_scores, sbr_mask_scores_shard, sbr_topk_rows, sbr_merge_topk,
sbr_rank_metrics) through the C ABI against the plain references of tests/evalk_ref.py, and FullEvaluator.eval_topk / get_results
against a host restatement built from them. The header of evalk_ref.py states the ordering rule (NaN first, -0 == +0, ties by ascending
index), the float64 metric definitions and the derivation of the NDCG bound; tests/test_evalk_refs_cpu.py proves the references on the
very inputs generated here and shows that the listed wrong kernels are rejected by the checks used here.

Conventions of this file
  * Every fp32 / int32 operand and every output lives in a NaN-filled guarded buffer (hip_testutil._Buf; int32 data through a bit
    view, so an int32 guard element reads as item 2,143,289,344): a write outside the result fails the test, a read outside poisons
    it. The int64 user ids and CSR row pointers are plain device tensors (read-only, no fp32 view of them exists).
  * Lists are compared by evalk_ref.same_lists: values "same NaN-ness, else ==", indices exactly. Mask results compare bit for bit.
  * sbr_topk_rows: I < 8,192 and I > 65,536 run the radix kernel, 8,192 <= I <= 65,536 the sampled one (k <= 256 always fits its
    candidate rule 8 k <= 2,048). The sampled kernel takes 16-byte loads only for a row whose base is 16-byte aligned: every
    I >= 8,192 also runs one float into the allocation with an odd row stride (rows 0, 1, 2, 4, 5, 6 of eight then start unaligned:
    the scalar collection loop) and aligned with ld = I + 4; all three layouts must return the same bits.
  * NDCG is checked with evalk_ref.check_metrics, which prints nothing; every test prints its worst error / bound (pytest -s)."""
import ctypes
import types

import numpy as np
import pytest
import torch

import evalk_ref as E
from hip_testutil import DEV, U32, S, _L, _assert_bits, _bits, _Buf, _i32, _i64, _p, call, stream

pytestmark = pytest.mark.gpu

TOPK_I_RADIX = [1, 2, 255, 256, 257, 3299, 8191]
TOPK_I_SAMPLED = [8192, 8193, 8207, 8448 + 5, 65535, 65536]      # 8207 % 256 = 15, 8453 % 256 = 5: a short last sample line
TOPK_I_LONG = [65537]
TOPK_KS = [1, 2, 31, 32, 33, 255, 256]
ROW_KINDS = ('random', 'heavy_ties', 'constant', 'all_neg_inf_but_three', 'half_neg_inf', 'ascending', 'descending', 'denormals',
             'max_overflows_the_candidates', 'signed_zeros', 'nans_scattered', 'all_nan')
ROW_GROUPS = (ROW_KINDS[:8], ROW_KINDS[4:])                      # eight rows per launch; together every kind at every I

MASK_I, MASK_U = 300, 264
MASK_BU = [1, 3, 4, 5, 257]
MASK_WINDOWS = [(0, 100), (120, 57), (37, 1), (MASK_I - 1, 1), (0, MASK_I)]      # [off, off + n) of the shard form

MERGE_SHAPES = [(1, 1), (1, 256), (2, 128), (4, 64), (8, 32), (3, 85), (7, 1), (5, 13), (2, 32)]      # W * k of 64, 65, 255 and 256 among them
MERGE_BU = [1, 5, 257]

METRIC_I = 600
METRIC_BU = [1, 255, 256, 257]
METRIC_KMAX = [1, 20, 256]
EVAL_KS = [1, 2, 3, 5, 8, 10, 15, 20, 30, 50, 64]                # eleven cut-offs: two sbr_rank_metrics launches per eval_topk
EVAL_METRICS = ['ndcg', 'recall', 'precision', 'hitrate', 'f_score', 'coverage']


# ---- case generators (also imported by tests/test_evalk_refs_cpu.py; no GPU needed) -------------------------------------------
def _from_bits(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)


def topk_row(kind, I, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(I).astype(np.float32)
    if kind == 'heavy_ties':
        x = (rng.integers(0, 8, I) / 4).astype(np.float32)
    elif kind == 'constant':
        x[:] = 1.5
    elif kind == 'all_neg_inf_but_three':
        x[:] = -np.inf
        pos = rng.choice(I, size=min(3, I), replace=False)
        x[pos] = np.float32([1., 1., 2.])[:len(pos)]
    elif kind == 'half_neg_inf':
        x[rng.random(I) < 0.5] = -np.inf
    elif kind == 'ascending':
        x = (np.arange(I) * 0.25 - 100).astype(np.float32)
    elif kind == 'descending':
        x = (np.arange(I)[::-1] * 0.25 - 100).astype(np.float32)
    elif kind == 'denormals':                                    # 4,095 distinct magnitudes below 2^-137, both signs: ties too
        x = _from_bits(rng.integers(1, 1 << 12, I).astype(np.uint32) | (rng.integers(0, 2, I).astype(np.uint32) << 31)).copy()
    elif kind == 'max_overflows_the_candidates':                 # 3,000 (> 2,048) elements tie at the maximum once I >= 6,000
        x[rng.choice(I, size=min(max(I // 2, 1), 3000), replace=False)] = 7.0
    elif kind == 'signed_zeros':
        x = np.where(rng.random(I) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        x[rng.choice(I, size=min(I // 8, 5), replace=False)] = -1.0
        x[0] = -0.0                                              # the lowest index is a -0: it leads the zeros
    elif kind == 'nans_scattered':
        b = x.view(np.uint32).copy()
        pos = np.sort(rng.choice(I, size=max(I // 16, min(I, 2)), replace=False))
        b[pos[0::2]] = E.NAN_NEG                                 # the first NaN by index has its sign bit set
        b[pos[1::2]] = E.NAN_POS
        x = _from_bits(b).copy()
    elif kind == 'all_nan':
        x = _from_bits(np.where(np.arange(I) % 2 == 0, E.NAN_NEG, E.NAN_POS)).copy()
    else:
        assert kind == 'random'
    return x


def topk_rows_input(I, group):
    """fp32 [8, I]: one row of every kind of ROW_GROUPS[group]"""
    return torch.from_numpy(np.stack([topk_row(kind, I, 1000 * I + 16 * group + j) for j, kind in enumerate(ROW_GROUPS[group])]))


def topk_ks(I):
    return sorted({min(k, I) for k in TOPK_KS})


def mask_world():
    """exclusion CSR over MASK_U users and MASK_I items; by u % 6: first / last column, empty, 70 entries, 140 entries, five, the last
    column only -> (indptr int64, indices int32)"""
    rng = np.random.default_rng(5)
    rows = []
    for u in range(MASK_U):
        n = {0: 3, 1: 0, 2: 70, 3: 140, 4: 5, 5: 1}[u % 6]
        c = np.sort(rng.choice(np.arange(1, MASK_I - 1), size=n, replace=False))
        if u % 6 == 0:
            c[0], c[-1] = 0, MASK_I - 1
        if u % 6 == 5:
            c[0] = MASK_I - 1
        rows.append(c)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32)


def mask_case(Bu, permuted):
    """-> (scores fp32 [Bu, MASK_I], u_idx int64 [Bu] or None)"""
    rng = np.random.default_rng(100 * Bu + permuted)
    scores = torch.from_numpy(rng.standard_normal((Bu, MASK_I)).astype(np.float32))
    if not permuted:
        return scores, None
    u = rng.integers(0, MASK_U, Bu)
    u[0] = 3                                                     # the 140-entry row
    if Bu >= 3:
        u[1], u[2] = 2, 3                                        # the 70-entry row, and a repeat
    return scores, u.astype(np.int64)


def merge_case(W, Bu, k, seed=0):
    """-> (vals fp32 [W, Bu, k], idxs int32 [W, Bu, k]): per-shard lists, score descending with many ties across shards (multiples of
    1/8, zeros of both signs), shard w owning the items [1000 w, 1000 w + 1000); 0 .. k valid entries per (shard, user), the rest
    (-inf, -1); users b % 7 == 3 have no entry at all; for b % 5 == 1 the last valid entry of every shard scores -inf; for b % 11 == 5
    the first entry of shard 0 is a NaN with the sign bit set and that of shard 1 a NaN with it clear"""
    rng = np.random.default_rng(1000 * W + 10 * k + Bu + seed)
    vals = -np.sort(-(rng.integers(0, 40, (W, Bu, k)) / 8).astype(np.float32), axis=2)
    vals[(vals == 0) & (rng.random(vals.shape) < 0.5)] = -0.0
    idxs = (np.argsort(rng.random((W, Bu, 1000)), axis=2)[:, :, :k] + 1000 * np.arange(W)[:, None, None]).astype(np.int32)
    n_valid = rng.integers(0, k + 1, (W, Bu))
    b = np.arange(Bu)
    n_valid[:, b % 7 == 3] = 0
    bits = vals.view(np.uint32)
    for w in range(W):
        for u in b[(b % 5 == 1)]:
            if n_valid[w, u] > 0:
                vals[w, u, n_valid[w, u] - 1] = -np.inf
        if w < 2:
            for u in b[(b % 11 == 5)]:
                if n_valid[w, u] > 0:
                    bits[w, u, 0] = E.NAN_NEG if w == 0 else E.NAN_POS
    empty = np.arange(k)[None, None, :] >= n_valid[..., None]
    vals[empty] = -np.inf
    idxs[empty] = -1
    return torch.from_numpy(vals), torch.from_numpy(idxs)


def metric_ks_sets(kmax):
    """[1], [kmax], eight ascending cut-offs, and a set whose largest is below kmax"""
    return {1: [[1]], 20: [[1], [20], [1, 2, 3, 5, 8, 10, 15, 20], [3, 10]],
            256: [[1], [256], [1, 2, 5, 10, 20, 50, 100, 256], [5, 100]]}[kmax]


def _build_list(rng, pos, n_items, kmax, kind):
    """one ranked list of kmax item ids; kind: 0 mixed (a positive with p = 0.5 per rank), 1 perfect, 2 mixed with a -1 tail,
    3 mixed with the first positive listed twice (ndcg above 1 before the clamp), 4 no hit, 5 mixed with p = 0.2"""
    pos = rng.permutation(pos)
    neg = rng.permutation(np.setdiff1d(np.arange(n_items), pos))
    p = {0: 0.5, 1: 1.0, 2: 0.5, 3: 0.5, 4: 0.0, 5: 0.2}[kind]
    out, ip, ineg = np.empty(kmax, dtype=np.int32), 0, 0
    for r in range(kmax):
        if ip < len(pos) and rng.random() < p:
            out[r], ip = pos[ip], ip + 1
        else:
            out[r], ineg = neg[ineg], ineg + 1
    if kind == 2:
        out[int(rng.integers(0, kmax + 1)):] = -1
    if kind == 3 and len(pos) and kmax >= 2:
        out[0] = out[1] = pos[0]
    return out


def _label_rows(rng, n_rows, n_items, kmax):
    """label rows by (u + 1) % 12: 0 -> no positive; else npos cycles through 1, kmax - 1, kmax, kmax + 5 and a random 2 .. 30. Rows
    u % 3 == 0 hold item 0, rows u % 3 == 1 the last item"""
    rows = []
    for u in range(n_rows):
        if (u + 1) % 12 == 0:
            rows.append(np.zeros(0, dtype=np.int32))
            continue
        npos = [1, max(kmax - 1, 1), kmax, kmax + 5, int(rng.integers(2, 31))][u % 5]
        c = rng.choice(np.arange(1, n_items - 1), size=npos, replace=False)
        if u % 3 == 0:
            c[0] = 0
        elif u % 3 == 1:
            c[0] = n_items - 1
        rows.append(np.sort(c).astype(np.int32))
    return rows


def _csr(rows):
    return (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64),
            (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32))


def metrics_world(Bu, kmax, permuted):
    """-> (topk_idx int32 [Bu, kmax], u_idx int64 [Bu] or None, (indptr, indices)); the lists are built against the label row of the
    user they belong to, list kinds by b % 6 (``_build_list``)"""
    rng = np.random.default_rng(10000 * Bu + 10 * kmax + permuted)
    U = Bu + 9
    rows = _label_rows(rng, U, METRIC_I, kmax)
    if permuted:
        u = rng.integers(0, U, Bu)
        u[-1] = u[0]
        if Bu == 1:
            u[0] = 3
    else:
        u = np.arange(Bu)
    top = np.stack([_build_list(rng, rows[u[b]], METRIC_I, kmax, b % 6) for b in range(Bu)])
    return torch.from_numpy(top), (u.astype(np.int64) if permuted else None), _csr(rows)


def metrics_inputs():
    """every (topk_idx, u_idx, csr, ks) the metric test below feeds the kernel, with a label"""
    for Bu in METRIC_BU:
        for kmax in METRIC_KMAX:
            for permuted in (False, True):
                top, u, csr = metrics_world(Bu, kmax, permuted)
                for ks in metric_ks_sets(kmax):
                    yield f'Bu {Bu} kmax {kmax} {"permuted" if permuted else "identity"} ks {ks}', top, u, csr, ks


def evaluator_world():
    """A split of 500 of 560 items and 300 users -> (dataset stand-in, [(u_idxs int64, topk positions int32 [Bu, 64])] for two eval_topk
    calls that overlap in 20 users, label CSR over (user id, position in the split))"""
    rng = np.random.default_rng(77)
    n_users, n_all, n_split, kmax = 300, 560, 500, max(EVAL_KS)
    import scipy.sparse as sp
    items = np.sort(rng.choice(n_all, size=n_split, replace=False))
    rows = _label_rows(rng, n_users, n_split, 20)                # positions in the split
    indptr, indices = _csr(rows)
    split = sp.csr_matrix((np.ones(len(indices), dtype=np.float32), indices, indptr), shape=(n_users, n_split))
    full = np.zeros((n_users, n_all), dtype=np.float32)
    full[:, items] = split.toarray()
    # interactions with items outside the split must not count
    outside = np.setdiff1d(np.arange(n_all), items)
    full[np.arange(n_users), outside[np.arange(n_users) % len(outside)]] = 1.0
    ds = types.SimpleNamespace(user_sampling_matrix=sp.csr_matrix(full), items_in_split=items, n_items_in_split=n_split)
    order = rng.permutation(n_users)
    calls = []
    for ids in (order[:160], order[140:]):
        top = np.stack([_build_list(rng, rows[u], n_split, kmax, j % 6) for j, u in enumerate(ids)])
        calls.append((ids.astype(np.int64), torch.from_numpy(top)))
    return ds, calls, (indptr, indices)


# ---- buffers ----------------------------------------------------------------------------------------------------------------------
def _fbuf(data, ld=None, off=0):
    """fp32 [rows, cols] data -> a guarded buffer holding exactly its bits (copied through an int32 view: NaN payloads survive)"""
    b = _Buf(data.shape[0], data.shape[1], ld=ld, off=off)
    b.t.view(torch.int32).copy_(_bits(data).to(DEV))
    return b


def _ibuf(data):
    """int32 [rows, cols] -> a guarded fp32 buffer holding the integers' bits"""
    b = _Buf(data.shape[0], data.shape[1])
    b.t.view(torch.int32).copy_(data.to(torch.int32).to(DEV))
    return b


def _all_nan(*bufs):
    return all(bool(torch.isnan(b.flat).all()) for b in bufs)


def _err():
    return _L().SibrarHipError


# ---- sbr_topk_rows ----------------------------------------------------------------------------------------------------------------
def _run_topk(scores, k, ld=None, off=0, what=''):
    Bu, I = scores.shape
    Sb, V, X = _fbuf(scores, ld=ld, off=off), _Buf(Bu, k), _Buf(Bu, k)
    call('sbr_topk_rows', Sb.ptr, Sb.ld, Bu, I, k, V.ptr, X.ptr, stream())
    _assert_bits(Sb.check_untouched(None, f'{what} scores'), scores, f'{what}: the scores changed')
    return V.check_untouched(None, f'{what} values').clone(), _bits(X.check_untouched(None, f'{what} indices')).clone()


def _assert_lists(got, want, kinds, what):
    bad = [r for r in range(len(kinds)) if not E.same_lists((got[0][r:r + 1], got[1][r:r + 1]), (want[0][r:r + 1], want[1][r:r + 1]))]
    if bad:
        r = bad[0]
        raise AssertionError(f'{what}: rows {[(b, kinds[b]) for b in bad]} differ from the stable descending order; row {r}: indices '
                             f'{got[1][r][:8].tolist()} ... expected {want[1][r][:8].tolist()} ..., values {got[0][r][:8].tolist()} ... '
                             f'expected {want[0][r][:8].tolist()} ...')


@pytest.mark.parametrize('I', TOPK_I_RADIX + TOPK_I_SAMPLED + TOPK_I_LONG)
def test_topk_rows_values_and_exact_indices(I):
    for group, kinds in enumerate(ROW_GROUPS):
        sc = topk_rows_input(I, group)
        full = E.topk_ref(sc, min(256, I))
        for k in topk_ks(I):
            what = f'I {I} k {k} group {group}'
            got = _run_topk(sc, k, what=what)
            _assert_lists(got, (full[0][:, :k], full[1][:, :k]), kinds, what)
            if I >= 8192:
                odd = (I | 1) if (I | 1) > I else I + 2
                for ld, off, name in ((odd, 1, 'one float in, odd ld'), (I + 4, 0, 'aligned, ld = I + 4')):
                    other = _run_topk(sc, k, ld=ld, off=off, what=f'{what} {name}')
                    _assert_bits(other[0], got[0], f'{what} {name}: values differ from the contiguous run')
                    assert torch.equal(other[1], got[1]), f'{what} {name}: indices differ from the contiguous run'


def test_topk_rows_refusals_write_nothing():
    sc = _fbuf(topk_rows_input(257, 0))
    for I, k in ((257, 0), (257, 257), (3, 4)):
        V, X = _Buf(8, 8), _Buf(8, 8)
        with pytest.raises(_err(), match='sbr_topk_rows'):
            call('sbr_topk_rows', sc.ptr, sc.ld, 8, I, k, V.ptr, X.ptr, stream())
        assert _all_nan(V, X), f'I {I} k {k}: a refused call wrote'
    V, X = _Buf(8, 8), _Buf(8, 8)
    call('sbr_topk_rows', sc.ptr, sc.ld, 0, 257, 5, V.ptr, X.ptr, stream())        # Bu = 0: nothing to do, no error
    assert _all_nan(V, X)


def test_topk_rows_through_ops_on_a_strided_view():
    """ops.topk_rows passes the view's row stride: a column slice of a wider matrix gives the lists of its contiguous copy"""
    sc = topk_rows_input(8207, 1)
    wide = _fbuf(torch.cat([sc, sc.flip(1)], dim=1))
    val, idx = S().ops.topk_rows(wide.t[:, :8207], 33)
    want = E.topk_ref(sc, 33)
    _assert_lists((val.cpu(), idx.cpu()), want, ROW_GROUPS[1], 'ops.topk_rows on a view')


# ---- sbr_mask_scores / sbr_mask_scores_shard --------------------------------------------------------------------------------------
@pytest.mark.parametrize('Bu', MASK_BU)
def test_mask_scores_and_the_shard_form(Bu):
    csr = mask_world()
    indptr, indices = _i64(csr[0]), _i32(csr[1])
    for permuted in (False, True):
        scores, u = mask_case(Bu, permuted)
        u_d = None if u is None else _i64(u)
        what = f'Bu {Bu} {"permuted" if permuted else "NULL u_idx"}'
        B = _fbuf(scores, ld=MASK_I + 3)
        call('sbr_mask_scores', B.ptr, B.ld, _p(u_d), indptr.data_ptr(), indices.data_ptr(), Bu, stream())
        _assert_bits(B.check_untouched(None, what), E.mask_ref(scores, u, csr), what)
        for off, n in MASK_WINDOWS:
            part = scores[:, off:off + n].contiguous()
            B = _fbuf(part, ld=n + 5)
            call('sbr_mask_scores_shard', B.ptr, B.ld, _p(u_d), indptr.data_ptr(), indices.data_ptr(), Bu, off, n, stream())
            _assert_bits(B.check_untouched(None, f'{what} window {off}+{n}'), E.mask_ref(part, u, csr, item_offset=off), f'{what} window {off}+{n}')
        # the wrapper: entry point chosen by item_offset, row stride and width taken from the view
        if u_d is not None:
            ops = S().ops
            B = _fbuf(scores, ld=MASK_I + 3)
            ops.mask_scores_(B.t, u_d, indptr, indices)
            _assert_bits(B.check_untouched(None, what), E.mask_ref(scores, u, csr), f'{what} ops')
            part = scores[:, 120:177].contiguous()
            B = _fbuf(part, ld=64)
            ops.mask_scores_(B.t, u_d, indptr, indices, item_offset=120)
            _assert_bits(B.check_untouched(None, what), E.mask_ref(part, u, csr, item_offset=120), f'{what} ops shard')


# ---- sbr_merge_topk ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('W,k', MERGE_SHAPES)
def test_merge_topk_values_and_exact_indices(W, k):
    for Bu in MERGE_BU:
        vals, idxs = merge_case(W, Bu, k)
        Vb, Xb = _fbuf(vals.view(W * Bu, k)), _ibuf(idxs.view(W * Bu, k))
        V, X = _Buf(Bu, k), _Buf(Bu, k)
        call('sbr_merge_topk', Vb.ptr, Xb.ptr, W, Bu, k, V.ptr, X.ptr, stream())
        what = f'W {W} k {k} Bu {Bu}'
        _assert_bits(Vb.check_untouched(None, what), vals.view(W * Bu, k), f'{what}: the input values changed')
        got = (V.check_untouched(None, f'{what} values'), _bits(X.check_untouched(None, f'{what} indices')))
        want = E.merge_ref(vals, idxs, k)
        bad = [b for b in range(Bu) if not E.same_lists((got[0][b:b + 1], got[1][b:b + 1]), (want[0][b:b + 1], want[1][b:b + 1]))]
        assert not bad, (f'{what}: {len(bad)} users differ, first {bad[0]}: indices {got[1][bad[0]][:8].tolist()} expected '
                         f'{want[1][bad[0]][:8].tolist()}, values {got[0][bad[0]][:8].tolist()} expected {want[0][bad[0]][:8].tolist()}')


def test_merge_topk_refuses_more_than_256_entries():
    vals, idxs = merge_case(2, 5, 128)
    Vb, Xb, V, X = _fbuf(vals.view(10, 128)), _ibuf(idxs.view(10, 128)), _Buf(5, 8), _Buf(5, 8)
    with pytest.raises(_err(), match='sbr_merge_topk'):
        call('sbr_merge_topk', Vb.ptr, Xb.ptr, 257, 5, 1, V.ptr, X.ptr, stream())
    assert _all_nan(V, X)


# ---- sbr_rank_metrics -------------------------------------------------------------------------------------------------------------
def _rank_metrics(T, kmax, u_d, indptr, indices, Bu, ks, O):
    arr = (ctypes.c_int * len(ks))(*ks)
    call('sbr_rank_metrics', T.ptr, kmax, _p(u_d), indptr.data_ptr(), indices.data_ptr(), Bu, ctypes.cast(arr, ctypes.c_void_p), len(ks),
         O.ptr, stream())


@pytest.mark.parametrize('kmax', METRIC_KMAX)
@pytest.mark.parametrize('Bu', METRIC_BU)
def test_rank_metrics_against_float64(Bu, kmax):
    worst = 0.0
    for permuted in (False, True):
        top, u, csr = metrics_world(Bu, kmax, permuted)
        T, u_d, indptr, indices = _ibuf(top), (None if u is None else _i64(u)), _i64(csr[0]), _i32(csr[1])
        for ks in metric_ks_sets(kmax):
            what = f'Bu {Bu} kmax {kmax} {"permuted" if permuted else "identity"} ks {ks}'
            O = _Buf(3 * len(ks), Bu)
            _rank_metrics(T, kmax, u_d, indptr, indices, Bu, ks, O)
            got = O.check_untouched(None, what).reshape(3, len(ks), Bu)
            worst = max(worst, E.check_metrics(got, top, u, csr, ks, what))
        assert torch.equal(_bits(T.check_untouched(None, 'lists')), top), 'the lists changed'
    print(f'ndcg err / bound, worst over Bu {Bu} kmax {kmax}: {worst:.4f}')


def test_rank_metrics_refusals_write_nothing():
    top, u, csr = metrics_world(5, 20, False)
    T, indptr, indices = _ibuf(top), _i64(csr[0]), _i32(csr[1])
    for ks in ([1, 2, 3, 4, 5, 6, 7, 8, 9], [5, 3], [3, 3], [1, 21]):
        O = _Buf(3 * len(ks), 5)
        with pytest.raises(_err(), match='sbr_rank_metrics'):
            _rank_metrics(T, 20, None, indptr, indices, 5, ks, O)
        assert _all_nan(O), f'ks {ks}: a refused call wrote'


# ---- FullEvaluator ----------------------------------------------------------------------------------------------------------------
def evaluator_expectation(calls, csr):
    """The host restatement: -> ({key: (float64 per-user values, per-user bound)}, {coverage key: value}) for EVAL_KS over the users of
    all calls in call order. ndcg / recall / precision from evalk_ref; hit rate = hits > 0; F-score 2 p r / (p + r) with 0 / 0 -> 0;
    coverage = distinct non-negative ids among the first k entries / items in the split.
    Per-user bounds: ndcg evalk_ref.ndcg_bound; recall and precision one rounding (u |x|; the GPU module also checks them bit for
    bit); hit rate 0; F-score 6 u |f| (p^ and r^ carry one rounding each, which enter the numerator once each and the denominator at
    most once; product, sum and division round once each), with evalk_ref's margin."""
    u = U32
    ref = torch.cat([E.metrics_ref64(top, ids, csr, EVAL_KS) for ids, top in calls], dim=2).numpy()
    nb = torch.cat([E.ndcg_bound(top, ids, csr, EVAL_KS) for ids, top in calls], dim=1).numpy()
    per_user = {}
    for q, k in enumerate(EVAL_KS):
        nd, rc, pr = ref[0, q], ref[1, q], ref[2, q]
        den = pr + rc
        f = np.where(den > 0, 2 * pr * rc / np.where(den > 0, den, 1.0), 0.0)
        per_user[f'ndcg@{k}'] = (nd, nb[q])
        per_user[f'recall@{k}'] = (rc, u * rc)
        per_user[f'precision@{k}'] = (pr, u * pr)
        per_user[f'hitrate@{k}'] = ((pr > 0).astype(np.float64), np.zeros_like(pr))
        per_user[f'f_score@{k}'] = (f, E.MARGIN * 6 * u * f + E.TINY)
    tops = np.concatenate([top.numpy() for _, top in calls])
    coverage = {}
    for k in EVAL_KS:
        ids = tops[:, :k].reshape(-1)
        coverage[f'coverage@{k}'] = len(set(ids[ids >= 0].tolist())) / 500
    return per_user, coverage


def test_full_evaluator_against_the_host_restatement():
    """eval_topk twice, then get_results: every per-user array inside its bound, every mean within mean(bound) + 16 u |mean| and every
    _std within max(bound) + 16 u std + 16 u of the float64 figures (an fp32 pairwise mean of 320 values in [0, 1] errs by less than
    16 u of it; the population standard deviation moves by at most the largest per-user error, and its fp32 evaluation — mean,
    differences with an absolute error below 11 u, squares, mean, root — by less than 16 u (1 + std)); coverage exactly; the keys in
    natural order; two sbr_rank_metrics launches per eval_topk for the eleven cut-offs."""
    from oracle import eval_ref
    ds, calls, csr = evaluator_world()
    ev = S().FullEvaluator(config=types.SimpleNamespace(top_k=list(EVAL_KS), metrics=list(EVAL_METRICS), calculate_std=True), dataset=ds)
    lib = _L()
    lib.CALL_LOG = []
    try:
        for ids, top in calls:
            ev.eval_topk(_i64(ids), _ibuf(top).t.view(torch.int32))
        launches = [args[7] for name, args in lib.CALL_LOG if name == 'sbr_rank_metrics']
    finally:
        lib.CALL_LOG = None
    assert launches == [8, 3, 8, 3], f'cut-offs per sbr_rank_metrics launch: {launches}'
    metrics, raw = ev.get_results(return_raw_results=True)
    per_user, coverage = evaluator_expectation(calls, csr)
    assert set(raw) == set(per_user)
    assert set(metrics) == set(per_user) | {f'{k}_std' for k in per_user} | set(coverage)
    assert list(metrics) == eval_ref.natural_sorted(list(metrics)), 'the keys are not in natural order'
    u, worst = U32, 0.0
    for key, (ref, bound) in per_user.items():
        got = raw[key].astype(np.float64)
        assert got.shape == ref.shape, key
        err = np.abs(got - ref)
        assert (err <= bound).all(), f'{key}: per-user values off by up to {err.max():.3e}'
        if key.startswith('ndcg'):
            worst = max(worst, float((err / bound).max()))
        m, s = float(ref.mean()), float(ref.std())
        assert abs(metrics[key] - m) <= bound.mean() + 16 * u * abs(m) + E.TINY, f'{key}: mean {metrics[key]!r}, expected {m!r}'
        assert abs(metrics[f'{key}_std'] - s) <= bound.max() + 16 * u * s + 16 * u, f'{key}_std: {metrics[key + "_std"]!r}, expected {s!r}'
    for key, c in coverage.items():
        assert metrics[key] == c, f'{key}: {metrics[key]!r}, expected {c!r}'
    print(f'FullEvaluator ndcg err / bound, worst: {worst:.4f}')
