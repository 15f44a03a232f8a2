"""Plain references for the rank-position metrics of csrc/topk.hip (sbr_rank_metrics_pos: dcg, ap, rr) and the inputs both test modules
feed them. numpy on the CPU; no fixtures, no pytest hooks, no GPU. tests/test_rank_pos_cpu.py proves the references on hand-worked
lists; tests/test_hip_rank_pos.py and tests/test_hip_eval_pos_metrics.py apply them to the kernel and to FullEvaluator.

(a) Definitions (``pos_metrics_ref64``, float64; include/sibrar_hip.h at sbr_rank_metrics_pos). Binary relevance, hits as in
    evalk_ref.hits_and_npos: hit[b, r] = topk[b, r] >= 0 and topk[b, r] in labels(u_b); h_r = the hits at ranks <= r; n_pos = |labels|.
      dcg@k = sum_{r < k, hit_r} 1 / log2(r + 2)
      ap@k  = (sum_{r < k, hit_r} h_r / (r + 1)) / min(k, n_pos)            (0 when n_pos == 0)
      rr@k  = 1 / (r0 + 1), r0 the smallest r < k with hit_r                 (0 without one)

(b) ``pos_metrics_f32``: rank_metrics_pos_kernel in numpy float32, one operation per line, in the kernel's order: on a hit at rank r,
    hits += 1; dcg += 1 / log2f(r + 2); apn += float(hits) / float(r + 1); the first hit's rank is kept. At r + 1 == ks[q]: dcg,
    apn / float(min(k, n_pos)), 1 / float(r0 + 1). Sums start from 0.f and take one addition per hit in ascending rank. ``disc`` replaces
    the discounts 1 / log2f(r + 2) by a given float32 vector (the device's own terms: the order of the sum is then pinned without
    pinning log2f, whose bits numpy and the device library need not share).

(c) Bounds on |fp32 - float64|, derived as evalk_ref.ndcg_bound derives its own (u = 2^-24 per fp32 operation, first order,
    LOG2_REL = the assumed relative error of log2f, MARGIN and TINY as there):
      dcg  a term is fl(1 / log2f(r + 2)): relative error <= LOG2_REL + u. The n_h hits are added one at a time from 0: the first
           addition is exact, each of the n_h - 1 others rounds a partial sum <= dcg:      |dcg^ - dcg| <= (LOG2_REL + u + (n_h - 1) u) dcg
      ap   a term is ONE correctly rounded division of two exactly converted integers (u); n_h - 1 rounding additions of partial sums
           <= the numerator; one more division by an exact integer (u):                      |ap^ - ap| <= (n_h + 1) u ap
      rr   one correctly rounded division:                                                    |rr^ - rr| <= u rr
    ap and rr involve no library function, so the kernel must equal ``pos_metrics_f32`` bit for bit there; the bounds on them serve the
    CPU proof of the restatement."""
import numpy as np

from evalk_ref import LOG2_REL, MARGIN, TINY, hits_and_npos
from hip_testutil import U32

N_ITEMS = 700                                # item ids of the kernel cases: enough negatives for a 300-entry list without a hit
POS_BU = [1, 4, 5, 257]                      # one wave, a full workgroup, one user into the next workgroup, many workgroups
POS_KMAX = [1, 63, 64, 65, 128, 130, 300]
N_KINDS, N_CLASSES = 8, 6


# ---- (a) float64 ------------------------------------------------------------------------------------------------------------------
def pos_metrics_ref64(topk_idx, u_idx, label_csr, ks):
    """-> float64 [3, n_ks, Bu]: dcg, ap, rr at every cut-off of ``ks``"""
    hit, npos = hits_and_npos(topk_idx, u_idx, label_csr)
    Bu, kmax = hit.shape
    r = np.arange(kmax, dtype=np.float64)
    h = np.cumsum(hit, axis=1).astype(np.float64)
    dcg_terms = hit / np.log2(r + 2.0)
    ap_terms = hit * h / (r + 1.0)
    out = np.zeros((3, len(ks), Bu), dtype=np.float64)
    has = npos > 0
    for q, k in enumerate(ks):
        assert 1 <= k <= kmax
        out[0, q] = dcg_terms[:, :k].sum(axis=1)
        out[1, q, has] = ap_terms[has, :k].sum(axis=1) / np.minimum(k, npos[has])
        any_hit = hit[:, :k].any(axis=1)
        out[2, q, any_hit] = 1.0 / (np.argmax(hit[:, :k], axis=1)[any_hit] + 1.0)
    return out


def idcg_ref64(npos, ks):
    """-> float64 [n_ks, Bu]: sum_{r < min(k, n_pos)} 1 / log2(r + 2), what turns dcg into ndcg"""
    npos = np.asarray(npos, dtype=np.int64)
    cum = np.concatenate([[0.0], np.cumsum(1.0 / np.log2(np.arange(2, max(ks) + 2, dtype=np.float64)))])
    return np.stack([cum[np.minimum(k, npos)] for k in ks])


# ---- (b) the kernel's arithmetic in numpy float32 ---------------------------------------------------------------------------------
def pos_metrics_f32(topk_idx, u_idx, label_csr, ks, disc=None):
    """rank_metrics_pos_kernel in numpy float32 -> float32 [3, n_ks, Bu]; ``disc``: float32 [>= kmax] discounts to use for 1 / log2f(r + 2)"""
    f = np.float32
    hit, npos = hits_and_npos(topk_idx, u_idx, label_csr)
    Bu, kmax = hit.shape
    out = np.full((3, len(ks), Bu), np.nan, dtype=f)
    dcg, apn = np.zeros(Bu, dtype=f), np.zeros(Bu, dtype=f)
    hits, first = np.zeros(Bu, dtype=np.int64), np.full(Bu, -1, dtype=np.int64)
    q = 0
    with np.errstate(all='ignore'):
        for r in range(kmax):
            if q >= len(ks):
                break
            if disc is None:
                x = f(r + 2)
                lg = np.log2(x)
                d = f(1.0) / lg
                assert lg.dtype == f
            else:
                d = np.asarray(disc, dtype=f)[r]
            assert d.dtype == f
            h = hit[:, r]
            hits = hits + h
            dcg = np.where(h, dcg + d, dcg)
            term = hits.astype(f) / f(r + 1)
            apn = np.where(h, apn + term, apn)
            first = np.where(h & (first < 0), r, first)
            while q < len(ks) and ks[q] == r + 1:
                den = np.minimum(ks[q], npos).astype(f)
                ap = apn / den
                rr = f(1.0) / (first + 1).astype(f)
                out[0, q] = dcg
                out[1, q] = np.where(npos > 0, ap, f(0.0))
                out[2, q] = np.where(first >= 0, rr, f(0.0))
                q += 1
    assert q == len(ks), 'ks must be ascending and <= kmax'
    assert out.dtype == f and dcg.dtype == f and apn.dtype == f and term.dtype == f
    return out


# ---- (c) bounds -------------------------------------------------------------------------------------------------------------------
def _hits_below(topk_idx, u_idx, label_csr, ks):
    hit, _ = hits_and_npos(topk_idx, u_idx, label_csr)
    return np.stack([hit[:, :k].sum(axis=1) for k in ks])


def dcg_bound(topk_idx, u_idx, label_csr, ks):
    """-> float64 [n_ks, Bu]: the bound of (c) on |fp32 dcg - pos_metrics_ref64(...)[0]|"""
    n_h = _hits_below(topk_idx, u_idx, label_csr, ks)
    dcg = pos_metrics_ref64(topk_idx, u_idx, label_csr, ks)[0]
    return MARGIN * dcg * (LOG2_REL + U32 + (np.maximum(n_h, 1) - 1) * U32) + TINY


def ap_rr_bounds(topk_idx, u_idx, label_csr, ks):
    """-> float64 [2, n_ks, Bu]: the bounds of (c) on the fp32 restatement's ap and rr"""
    n_h = _hits_below(topk_idx, u_idx, label_csr, ks)
    ref = pos_metrics_ref64(topk_idx, u_idx, label_csr, ks)
    return np.stack([MARGIN * ref[1] * (n_h + 1) * U32 + TINY, MARGIN * ref[2] * U32 + TINY])


# ---- inputs of the kernel tests ---------------------------------------------------------------------------------------------------
def pos_ks_sets(kmax):
    """cut-off sets per list length: 1, 64, 65 and kmax where they fit (inside a step, on a step edge, in the partial last step), kmax
    alone (steps without a cut-off), eight cut-offs, several in one step, a step that is skipped, and a largest cut-off below kmax"""
    return {1: [[1]],
            63: [[1, 5, 63], [63], [2, 10]],
            64: [[1, 10, 64], [64]],
            65: [[1, 64, 65], [65], [3, 64]],
            128: [[1, 2, 63, 64, 65, 100, 127, 128], [64, 128], [65]],
            130: [[1, 64, 65, 128, 129, 130], [130], [5, 100]],
            300: [[1, 64, 65, 128, 192, 193, 256, 300], [300], [70, 200]]}[kmax]


def label_rows(rng, n_rows, kmax):
    """label rows by u % 6: 0 -> none; 1 -> one; 2 -> kmax + 5 (more than any cut-off); 3 -> kmax; 4 -> a random 2 .. 30;
    5 -> max(kmax - 1, 1). Rows u % 3 == 0 hold item 0, rows u % 3 == 1 the last item"""
    rows = []
    for u in range(n_rows):
        npos = [0, 1, kmax + 5, kmax, int(rng.integers(2, 31)), max(kmax - 1, 1)][u % N_CLASSES]
        c = rng.choice(np.arange(1, N_ITEMS - 1), size=npos, replace=False)
        if npos and u % 3 == 0:
            c[0] = 0
        elif npos and u % 3 == 1:
            c[0] = N_ITEMS - 1
        rows.append(np.sort(c).astype(np.int32))
    return rows


def build_list(rng, pos, kmax, kind, n_items=N_ITEMS):
    """one list of kmax distinct item ids against the label row ``pos``; kind: 0 a positive with p = 0.5 per rank, 1 every positive
    first, 2 as 0 with a -1 tail, 3 no hit, 4 hits at ranks 0, 63, 64 and the last one and nowhere else, 5 as 0 with p = 0.2, 6 one hit,
    at the last rank, 7 as 0 behind 70 ranks without a hit"""
    pos = rng.permutation(pos)
    neg = rng.permutation(np.setdiff1d(np.arange(n_items), pos))
    forced = {4: {0, 63, 64, kmax - 1}, 6: {kmax - 1}}.get(kind)
    p = {0: 0.5, 1: 1.0, 2: 0.5, 3: 0.0, 5: 0.2, 7: 0.5}.get(kind, 0.0)
    out, ip, ineg = np.empty(kmax, dtype=np.int32), 0, 0
    for r in range(kmax):
        want = (r in forced) if forced is not None else (rng.random() < p and not (kind == 7 and r < min(70, kmax - 1)))
        if want and ip < len(pos):
            out[r], ip = pos[ip], ip + 1
        else:
            out[r], ineg = neg[ineg], ineg + 1
    if kind == 2:
        out[int(rng.integers(0, kmax + 1)):] = -1
    return out


def csr_of(rows):
    return (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64),
            (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32))


def pos_world(Bu, kmax, permuted):
    """-> (topk_idx int32 [Bu, kmax], u_idx int64 [Bu] or None, (indptr, indices)). List b is built against the label row of its user;
    its kind is (b + kmax) % 8 and, with u_idx None, its label class b % 6, so that many users meet every (kind, class) pair and the
    one-user cases differ by kmax. ``permuted``: random user ids with repeats (the last user is the first one again)."""
    rng = np.random.default_rng(20000 * Bu + 20 * kmax + permuted)
    U = Bu + 9
    rows = label_rows(rng, U, kmax)
    if permuted:
        u = rng.integers(0, U, Bu)
        u[-1] = u[0]
        if Bu == 1:
            u[0] = 3 + kmax % 6
    else:
        u = np.arange(Bu)
    top = np.stack([build_list(rng, rows[u[b]], kmax, (b + kmax) % N_KINDS) for b in range(Bu)])
    return top, (u.astype(np.int64) if permuted else None), csr_of(rows)


def branches_met(top, u, csr):
    """-> the set of named branches a case's lists reach (what the kernel tests assert over their regenerated inputs)"""
    hit, npos = hits_and_npos(top, u, csr)
    kmax = hit.shape[1]
    n_hits = hit.sum(axis=1)
    met = set()
    for name, cond in (('hit at rank 0', hit[:, 0].any()), ('hit at rank 63', kmax > 63 and hit[:, 63].any()),
                       ('hit at rank 64', kmax > 64 and hit[:, 64].any()), ('hit at the last rank', hit[:, -1].any()),
                       ('the whole list hits', (n_hits == kmax).any()), ('no hit with positives', ((n_hits == 0) & (npos > 0)).any()),
                       ('n_pos = 0', (npos == 0).any()), ('n_pos = 1', (npos == 1).any()), ('n_pos > kmax', (npos > kmax).any()),
                       ('n_pos < kmax', ((npos > 0) & (npos < kmax)).any()), ('padded with -1', (np.asarray(top) < 0).any()),
                       ('first hit past rank 64', (hit.any(axis=1) & (np.argmax(hit, axis=1) > 64)).any()),
                       ('user ids repeat', u is not None and len(set(u.tolist())) < len(u)), ('u_idx null', u is None)):
        if cond:
            met.add(name)
    return met


def branches_expected(kmax):
    """what the cases of one kmax must reach together (over POS_BU and both u_idx forms)"""
    want = {'hit at rank 0', 'hit at the last rank', 'the whole list hits', 'no hit with positives', 'n_pos = 0', 'n_pos = 1',
            'n_pos > kmax', 'padded with -1', 'user ids repeat', 'u_idx null'}
    if kmax > 63:
        want.add('hit at rank 63')
    if kmax > 64:
        want.add('hit at rank 64')
    if kmax > 2:
        want.add('n_pos < kmax')
    if kmax > 70:
        want.add('first hit past rank 64')
    return want


def single_hit_world(n):
    """n users with the one label item 0; user r's list holds it at rank r and -1 everywhere else: dcg@n of user r is the device's
    0.f + 1.f / log2f(r + 2), the term itself"""
    top = np.full((n, n), -1, dtype=np.int32)
    top[np.arange(n), np.arange(n)] = 0
    return top, None, csr_of([np.zeros(1, dtype=np.int32)] * n)


# ---- inputs of the evaluator test -------------------------------------------------------------------------------------------------
EVAL_KS = [1, 2, 3, 5, 8, 10, 15, 20, 30, 50, 70]                # eleven cut-offs (two launches of eight and three), one past rank 64


def evaluator_world():
    """A split of 400 of 450 items and 260 users -> (user_sampling_matrix, items_in_split, [(u_idxs, topk positions int32 [Bu, 70])] for
    two eval_topk calls that overlap in 20 users, label CSR over (user id, position in the split), user category int64 [260] in {0, 1})"""
    import scipy.sparse as sp
    rng = np.random.default_rng(91)
    n_users, n_all, n_split, kmax = 260, 450, 400, max(EVAL_KS)
    items = np.sort(rng.choice(n_all, size=n_split, replace=False))
    rows = []
    for u in range(n_users):
        npos = [0, 1, 75, 20, int(rng.integers(2, 31)), 5][u % N_CLASSES]
        rows.append(np.sort(rng.choice(n_split, size=npos, replace=False)).astype(np.int32))
    indptr, indices = csr_of(rows)
    full = np.zeros((n_users, n_all), dtype=np.float32)
    full[:, items] = sp.csr_matrix((np.ones(len(indices), dtype=np.float32), indices, indptr), shape=(n_users, n_split)).toarray()
    outside = np.setdiff1d(np.arange(n_all), items)
    full[np.arange(n_users), outside[np.arange(n_users) % len(outside)]] = 1.0       # interactions outside the split must not count
    order = rng.permutation(n_users)
    calls = []
    for ids in (order[:140], order[120:]):
        top = np.stack([build_list(rng, rows[u], kmax, j % N_KINDS, n_split) for j, u in enumerate(ids)])
        calls.append((ids.astype(np.int64), top))
    return sp.csr_matrix(full), items, calls, (indptr, indices), (np.arange(n_users) % 3 == 0).astype(np.int64)
