"""Plain references for the evaluation kernels (csrc/topk.hip): the exclusion mask, the per-row top-k, the merge of per-shard lists and
the ranking metrics. numpy / torch on the CPU; no fixtures, no pytest hooks, no GPU. tests/test_evalk_refs_cpu.py proves the references
and shows that each listed wrong kernel is rejected; tests/test_hip_evalk.py applies them to the kernels.

(a) The ordering rule (``topk_ref``, ``merge_ref``). A list is the first k of the STABLE DESCENDING order of the row:
      * every NaN, whatever its sign bit or payload, ranks ahead of +inf;
      * -0.0 and +0.0 are the same score;
      * equal scores (all NaNs are equal to each other, both zeros are equal) go in ascending index.
    This is what ``torch.sort(descending=True, stable=True)`` does. It is implemented here without torch.topk / torch.sort: every score
    is mapped to a canonical unsigned key (``sort_key``) and ``np.lexsort`` orders by (key descending, index ascending). Returned values
    are the row's own elements. Values are compared as "same NaN-ness, else ==" (``same_values``; -0 and +0 pass as equal, a NaN may
    come back with another sign or payload), indices exactly.

(b) The metrics (``metrics_ref64``): float64, from the definitions of oracle/eval_ref.py (eval/metrics.py:4-105) with binary relevance:
      hit[b, r] = topk[b, r] >= 0 and topk[b, r] in labels(u_b)          (one hit per list ENTRY: a repeated item counts again)
      recall@k = hits_k / npos (0 without positives),  precision@k = hits_k / k,
      ndcg@k   = min(1, sum_{r < k, hit} 1 / log2(r + 2)  /  sum_{r < min(k, npos)} 1 / log2(r + 2))     (0 without positives)

(c) ``metrics_f32``: rank_metrics_kernel in numpy float32, one operation per line, in the kernel's order: disc = 1 / log2f(r + 2);
    dcg += disc on a hit; idcg += disc while r < npos; at r + 1 == ks[q]: min(dcg / idcg, 1), hits / npos, hits / ks[q]. ``mutant``
    turns it into one of the wrong kernels of MUTANTS_METRICS.

(d) ``ndcg_bound``: per entry, |fp32 ndcg - metrics_ref64 ndcg| — derived, never fitted. u = 2^-24 per fp32 operation
    (hip_testutil.U32); every operation returns x (1 + d), |d| <= u, first order.
      L^   = log2f(r + 2)             r + 2 is exact in fp32; relative error <= LOG2_REL
      d^_r = fl(1 / L^)               a correctly rounded division (the build passes no fast-math flag):  relative error <= LOG2_REL + u
      dcg^ = the d^_r of the n_h hits added one at a time, starting from 0: the first addition is exact, each of the n_h - 1 others
             rounds a partial sum that is <= dcg (every term is positive):       |dcg^ - dcg| <= (LOG2_REL + u + (n_h - 1) u) dcg
      idcg^  the same over n_i = min(k, npos) ranks:                              |idcg^ - idcg| <= (LOG2_REL + u + (n_i - 1) u) idcg
      x^   = fl(dcg^ / idcg^)         one more u. With x = dcg / idcg:
             |x^ - x| <= x (2 LOG2_REL + 2 u + (max(n_h, 1) - 1) u + (n_i - 1) u + u)
      min(., 1) is 1-Lipschitz and is applied to both sides, so the clamped values differ by no more.
    (dcg and idcg share their d^_r, so much of the log2f error cancels in the quotient; the bound does not use that.)
    log2f: the ROCm installation this module was written against documents no accuracy figure for the device library's log2f (its
    share/ and doc trees were searched), so LOG2_ULP is an ASSUMPTION: 2 ulp, the allowance tests/hip_testutil.py (EXP_ULP) already
    makes for one expf / logf / tanhf call of the same library; one ulp is at most 2 u relative, hence LOG2_REL = 4 u.
    Every bound is multiplied by MARGIN = 1.125 and one fp32 subnormal is added — the margin of tests/optim_ref.py, for its reasons:
    the eighth pays for what first order drops (products of two roundings: a relative 2^-15 of the bound at the 256 ranks a list can
    have) and for the float64 evaluation of reference and bound, with room to spare. It was not sized to any measured kernel error.

Recall and precision carry no bound: each is ONE correctly rounded fp32 division of two small integers, so the kernel must return
np.float32(hits) / np.float32(den) bit for bit (``exact_recall_precision``). A perfect list — the first min(k, npos) entries all hits —
has dcg and idcg formed by the same additions in the same order: its NDCG must be exactly 1.0f (``perfect_pairs``)."""
import numpy as np
import torch

from hip_testutil import U32

LOG2_ULP = 2                                  # assumed accuracy of the device library's log2f, in ulp (see (d))
LOG2_REL = LOG2_ULP * 2 * U32
MARGIN = 1.125
TINY = 2.0 ** -149
NAN_POS, NAN_NEG = 0x7FC00000, 0xFFC00000     # the two quiet-NaN bit patterns the test rows are built from

MUTANTS_ORDER = ('ties_to_the_higher_index', 'negative_nan_last', 'plus_zero_ahead_of_minus_zero')
MUTANTS_METRICS = ('discount_log2_r_plus_1', 'ideal_dcg_over_k_ranks', 'precision_over_kmax', 'no_clamp', 'identity_label_rows',
                   'minus_one_is_item_zero')


def _np(x, dtype=None):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return a if dtype is None else np.ascontiguousarray(a, dtype=dtype)


# ---- (a) ordering ----------------------------------------------------------------------------------------------------------------
def sort_key(x, mutant=None):
    """fp32 array -> uint32 keys, larger key = ranks earlier: NaN (either sign) the largest, -0 the key of +0, otherwise the order of
    the reals with -inf the smallest"""
    x = _np(x, np.float32)
    b = x.view(np.uint32)
    neg = (b >> 31).astype(bool)
    key = np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    if mutant != 'plus_zero_ahead_of_minus_zero':
        key = np.where(x == 0, np.uint32(0x80000000), key)
    nan = np.isnan(x)
    if mutant == 'negative_nan_last':
        key = np.where(nan, np.where(neg, np.uint32(0), np.uint32(0xFFFFFFFF)), key)
    else:
        key = np.where(nan, np.uint32(0xFFFFFFFF), key)
    return key.astype(np.uint32)


def topk_ref(scores, k, mutant=None):
    """[B, I] fp32 -> (values [B, k] fp32, indices [B, k] int32): the first k of the stable descending order under the rule of (a)"""
    assert mutant is None or mutant in MUTANTS_ORDER
    s = _np(scores, np.float32)
    B, I = s.shape
    assert 1 <= k <= I
    idx = np.broadcast_to(np.arange(I, dtype=np.int64), (B, I))
    minor = -idx if mutant == 'ties_to_the_higher_index' else idx
    order = np.lexsort((minor, -sort_key(s, mutant).astype(np.int64)), axis=-1)[:, :k]
    return torch.from_numpy(np.take_along_axis(s, order, axis=1).copy()), torch.from_numpy(order.astype(np.int32))


def same_values(got, want):
    """same NaN-ness everywhere, == elsewhere (-0 == +0)"""
    got, want = _np(got, np.float32), _np(want, np.float32)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn)) and bool(np.array_equal(got[~gn], want[~wn]))


def same_lists(got, want):
    """(values, indices) pairs: values by ``same_values``, indices exactly"""
    return same_values(got[0], want[0]) and bool(np.array_equal(_np(got[1], np.int64), _np(want[1], np.int64)))


def mask_ref(scores, u_idx, csr, item_offset=None):
    """scores [Bu, n_cols] -> a copy with -inf wherever the CSR row of user u_idx[b] (row b when u_idx is None) names the column
    item_offset + c (item_offset None: 0); by dense boolean indexing"""
    indptr, indices = _np(csr[0], np.int64), _np(csr[1], np.int64)
    out = _np(scores, np.float32).copy()
    Bu, n_cols = out.shape
    off = 0 if item_offset is None else int(item_offset)
    n_all = max(int(indices.max()) + 1 if indices.size else 0, off + n_cols)
    dense = np.zeros((len(indptr) - 1, n_all), dtype=bool)
    dense[np.repeat(np.arange(len(indptr) - 1), np.diff(indptr)), indices] = True
    rows = np.arange(Bu) if u_idx is None else _np(u_idx, np.int64)
    out[dense[rows][:, off:off + n_cols]] = -np.inf
    return torch.from_numpy(out)


def floor_ref(scores, mu):
    """scores -> a copy with x[x < mu] = mu (the floor of the all-pairs evaluation form, applied before the mask); a NaN is not below mu
    and stays, mu in fp32"""
    out = _np(scores, np.float32).copy()
    out[out < np.float32(mu)] = np.float32(mu)
    return torch.from_numpy(out)


def merge_ref(vals, idxs, k):
    """vals / idxs [W, Bu, k'] -> (values [Bu, k] fp32, indices [Bu, k] int32): the W lists of a user concatenated; idx < 0 marks an
    empty slot; score descending (the keys of (a)), then item index ascending; empty slots last, as (-inf, -1)"""
    v, i = _np(vals, np.float32), _np(idxs, np.int64)
    W, Bu = v.shape[:2]
    v = np.concatenate(list(v), axis=1)
    i = np.concatenate(list(i), axis=1)
    assert k <= v.shape[1]
    empty = i < 0
    order = np.lexsort((i, -sort_key(v).astype(np.int64), empty), axis=-1)[:, :k]
    ov, oi, oe = (np.take_along_axis(a, order, axis=1) for a in (v, i, empty))
    return torch.from_numpy(np.where(oe, np.float32(-np.inf), ov).astype(np.float32)), torch.from_numpy(np.where(oe, -1, oi).astype(np.int32))


# ---- (b) metrics in float64 ------------------------------------------------------------------------------------------------------
def hits_and_npos(topk_idx, u_idx, label_csr, mutant=None):
    """-> (hit [Bu, kmax] bool, npos [Bu] int64) by a dense label matrix"""
    indptr, indices = _np(label_csr[0], np.int64), _np(label_csr[1], np.int64)
    top = _np(topk_idx, np.int64)
    Bu = top.shape[0]
    n_items = max(int(indices.max()) + 1 if indices.size else 1, int(top.max()) + 1, 1)
    dense = np.zeros((len(indptr) - 1, n_items), dtype=bool)
    dense[np.repeat(np.arange(len(indptr) - 1), np.diff(indptr)), indices] = True
    rows = np.arange(Bu) if (u_idx is None or mutant == 'identity_label_rows') else _np(u_idx, np.int64)
    y = dense[rows]
    hit = np.take_along_axis(y, np.maximum(top, 0), axis=1)
    if mutant != 'minus_one_is_item_zero':
        hit = hit & (top >= 0)
    return hit, y.sum(axis=1).astype(np.int64)


def metrics_ref64(topk_idx, u_idx, label_csr, ks):
    """-> float64 [3, n_ks, Bu]: ndcg, recall, precision at every cut-off of ``ks`` (see (b))"""
    hit, npos = hits_and_npos(topk_idx, u_idx, label_csr)
    Bu, kmax = hit.shape
    disc = 1.0 / np.log2(np.arange(2, kmax + 2, dtype=np.float64))
    cum_dcg = np.concatenate([np.zeros((Bu, 1)), np.cumsum(hit * disc, axis=1)], axis=1)
    cum_disc = np.concatenate([[0.0], np.cumsum(disc)])
    out = np.zeros((3, len(ks), Bu), dtype=np.float64)
    has = npos > 0
    for q, k in enumerate(ks):
        assert 1 <= k <= kmax
        h = hit[:, :k].sum(axis=1).astype(np.float64)
        idcg = cum_disc[np.minimum(k, npos)]
        out[0, q, has] = np.minimum(cum_dcg[has, k] / idcg[has], 1.0)
        out[1, q, has] = h[has] / npos[has]
        out[2, q] = h / k
    return torch.from_numpy(out)


# ---- (c) the kernel's arithmetic in numpy float32 ---------------------------------------------------------------------------------
def metrics_f32(topk_idx, u_idx, label_csr, ks, mutant=None):
    """rank_metrics_kernel in numpy float32 -> float32 [3, n_ks, Bu]"""
    f = np.float32
    assert mutant is None or mutant in MUTANTS_METRICS
    hit, npos = hits_and_npos(topk_idx, u_idx, label_csr, mutant)
    Bu, kmax = hit.shape
    out = np.full((3, len(ks), Bu), np.nan, dtype=f)
    dcg, idcg = np.zeros(Bu, dtype=f), np.zeros(Bu, dtype=f)
    hits = np.zeros(Bu, dtype=np.int64)
    q = 0
    with np.errstate(all='ignore'):
        for r in range(kmax):
            if q >= len(ks):
                break
            x = f(r + 1) if mutant == 'discount_log2_r_plus_1' else f(r + 2)
            lg = np.log2(x)
            disc = f(1.0) / lg
            assert lg.dtype == disc.dtype == f
            hits = hits + hit[:, r]
            dcg = np.where(hit[:, r], dcg + disc, dcg)
            ideal = np.full(Bu, True) if mutant == 'ideal_dcg_over_k_ranks' else (r < npos)
            idcg = np.where(ideal, idcg + disc, idcg)
            while q < len(ks) and ks[q] == r + 1:
                nd = dcg / idcg
                if mutant != 'no_clamp':
                    nd = np.minimum(nd, f(1.0))
                out[0, q] = np.where(npos > 0, nd, f(0.0))
                out[1, q] = np.where(npos > 0, hits.astype(f) / npos.astype(f), f(0.0))
                out[2, q] = hits.astype(f) / f(kmax if mutant == 'precision_over_kmax' else ks[q])
                q += 1
    assert out.dtype == f and dcg.dtype == f and idcg.dtype == f
    return out


# ---- (d) the bound and the exact parts -------------------------------------------------------------------------------------------
def ndcg_bound(topk_idx, u_idx, label_csr, ks):
    """-> float64 [n_ks, Bu]: the bound of (d) on |fp32 ndcg - metrics_ref64(...)[0]|"""
    u = U32
    hit, npos = hits_and_npos(topk_idx, u_idx, label_csr)
    Bu, kmax = hit.shape
    disc = 1.0 / np.log2(np.arange(2, kmax + 2, dtype=np.float64))
    cum_dcg = np.concatenate([np.zeros((Bu, 1)), np.cumsum(hit * disc, axis=1)], axis=1)
    cum_disc = np.concatenate([[0.0], np.cumsum(disc)])
    out = np.zeros((len(ks), Bu), dtype=np.float64)
    has = npos > 0
    for q, k in enumerate(ks):
        n_h = hit[:, :k].sum(axis=1)
        n_i = np.minimum(k, npos)
        x = np.zeros(Bu)
        x[has] = cum_dcg[has, k] / cum_disc[n_i[has]]                      # unclamped
        rel = 2 * LOG2_REL + 2 * u + (np.maximum(n_h, 1) - 1) * u + (np.maximum(n_i, 1) - 1) * u + u
        out[q] = x * rel
    return torch.from_numpy(MARGIN * out + TINY)


def exact_recall_precision(topk_idx, u_idx, label_csr, ks):
    """-> float32 [2, n_ks, Bu]: np.float32(hits) / np.float32(npos) (0 without positives) and np.float32(hits) / np.float32(k)"""
    f = np.float32
    hit, npos = hits_and_npos(topk_idx, u_idx, label_csr)
    out = np.zeros((2, len(ks), hit.shape[0]), dtype=f)
    has = npos > 0
    for q, k in enumerate(ks):
        h = hit[:, :k].sum(axis=1).astype(f)
        out[0, q, has] = h[has] / npos[has].astype(f)
        out[1, q] = h / f(k)
    return out


def perfect_pairs(topk_idx, u_idx, label_csr, ks):
    """-> bool [n_ks, Bu]: the first min(k, npos) entries are all hits, no other entry below k is, and the user has positives"""
    hit, npos = hits_and_npos(topk_idx, u_idx, label_csr)
    out = np.zeros((len(ks), hit.shape[0]), dtype=bool)
    r = np.arange(hit.shape[1])
    for q, k in enumerate(ks):
        want = r[None, :k] < np.minimum(k, npos)[:, None]
        out[q] = (npos > 0) & (hit[:, :k] == want).all(axis=1)
    return out


def check_metrics(got, topk_idx, u_idx, label_csr, ks, what=''):
    """The criterion both test modules apply to a [3, n_ks, Bu] fp32 result: NDCG inside ``ndcg_bound`` of ``metrics_ref64`` (NaN
    fails), exactly 1.0f on perfect lists, recall and precision bit-identical to one fp32 division. Raises AssertionError; -> the
    largest NDCG err / bound"""
    got = _np(got, np.float32)
    ref = metrics_ref64(topk_idx, u_idx, label_csr, ks).numpy()
    assert got.shape == ref.shape, f'{what}: shape {got.shape}, expected {ref.shape}'
    bound = ndcg_bound(topk_idx, u_idx, label_csr, ks).numpy()
    err = np.abs(got[0].astype(np.float64) - ref[0])
    bad = ~(err <= bound)
    assert not bad.any(), (f'{what}: ndcg outside the derived bound at {int(bad.sum())} of {bad.size} (cut-off, user) pairs, worst err '
                           f'{np.nan_to_num(err[bad], nan=np.inf).max():.3e} (bound there {bound[bad][0]:.3e})')
    perfect = perfect_pairs(topk_idx, u_idx, label_csr, ks)
    assert (got[0][perfect] == np.float32(1.0)).all(), f'{what}: a perfect list does not have ndcg == 1.0f exactly'
    exact = exact_recall_precision(topk_idx, u_idx, label_csr, ks)
    for j, nm in ((0, 'recall'), (1, 'precision')):
        diff = got[1 + j].view(np.int32) != exact[j].view(np.int32)
        assert not diff.any(), f'{what}: {nm} differs in bits from float32(hits) / float32(den) at {int(diff.sum())} of {diff.size} pairs'
    return float((err / bound).max())
