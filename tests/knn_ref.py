"""Float64 restatement of the neighbourhood models (csrc/knn.hip; utilities/similarities.py:18-130, algorithms/knn_algs.py:80-118), the fp32
error bound of a similarity value and the comparison rule of the g22 fixture. A plain module: no fixtures, no pytest hooks, no GPU.
tests/test_knn_cpu.py shows that the restatement meets the fixture recorded from the reference; tests/test_hip_knn.py applies restatement,
bound and rule to the kernels and the models.

(a) Restatement. X is a 0/1 matrix [n, m]; C = X X^T (integers), n_i = C_ii. For j != i with c = C_ij > 0
    cosine             v = c / (sqrt(n_i) sqrt(n_j))            jaccard        v = c / (n_i + n_j - c)
    asymmetric_cosine  v = c / (n_i^alpha n_j^(1 - alpha))      sorensen_dice  v = 2 c / (n_i + n_j)
    tversky            v = c / (c + alpha (n_i - c) + beta (n_j - c))
    value = v c / (c + shrinkage);   0 for every other pair.
The list of row i: its candidates by np.lexsort (value descending, index ascending), cut at k — the project's canonical rule. The reference
cuts with an unstable argsort instead; see (c). Predictions: UserKNN S M, ItemKNN M S^T with S the matrix of the lists.

(b) Bound — derived from the kernel's operation order (knn_value in csrc/knn.hip, the same order as in include/sibrar_hip.h), never fitted.
u = 2^-24. One fp32 operation returns x (1 + d), |d| <= u: +, *, / and sqrtf are correctly rounded in HIP device code (the compiler's
default for fp32 divide and sqrt), and nothing is contracted. Counts (c, n_i, n_j and the integer sums, all below 2^24) convert exactly.
alpha, beta and the shrinkage arrive as doubles rounded to fp32 once: one more (1 + d) each. All terms of a denominator are >= 0, so
relative errors do not grow in a sum. Roundings N per value, relative bound gamma_N = N u / (1 - N u):
    cosine             sqrtf, sqrtf, *, /                                        4
    jaccard            /                                                         1
    sorensen_dice      / (2 c is exact)                                          1
    tversky            fl(alpha), *, fl(beta), * (<= 2 on each term), +, +, /    5
    asymmetric_cosine  *, / and two powf calls; the ROCm tree states no accuracy for powf — ASSUMED here: 16 ulp = 32 u per call, the
                       limit OpenCL sets for pow, which the device library is built to meet. The exponents carry fl(alpha) and
                       fl(1 - fl(alpha)): |d alpha| <= u alpha, |d (1 - alpha)| <= u (alpha + |1 - alpha|), and d(n^e) / n^e = ln(n) de:
                                                                                 2 + 64 + alpha ln(n_i) + (alpha + |1 - alpha|) ln(n_j)
    shrinkage > 0      fl(shrinkage), +, /, *                                    4        (shrinkage = 0: c + 0, c / c and v * 1 are exact)

(c) The fixture rule. Which of several equal values at the k-th place the reference keeps is arbitrary, so
    k = 60   nothing is pruned in the 50 x 40 world: sim_mtx and the dense pred_mtx are compared in full;
    k = 5    the sorted values of every row are compared, and the index sets of the rows whose 5th and 6th candidate values differ by more
             than 1e-6 relative.
The reference zeroes the self similarity and may keep that explicit 0 in a short row: zeros are dropped from its rows first."""
import numpy as np
import scipy.sparse as sp

U32 = 2.0 ** -24
POWF_U = 32.0                     # assumed: 16 ulp per powf call, see (b)
SIMS = ('cosine', 'jaccard', 'asymmetric_cosine', 'tversky', 'sorensen_dice')
TIE_REL = 1e-6


def dense01(x):
    x = x.toarray() if sp.issparse(x) else np.asarray(x)
    return (x != 0).astype(np.int64)


def counts(x):
    """C = X X^T as int64 [n, n]"""
    if sp.issparse(x):
        x = sp.csr_matrix((np.ones(x.nnz, dtype=np.int64), x.nonzero()), shape=x.shape)
        return np.asarray((x @ x.T).todense())
    x = dense01(x)
    return x @ x.T


def _formula(cf, ni, nj, sim, shrinkage, alpha, beta):
    """elementwise (a) on float64 arrays of counts and row sizes"""
    if sim == 'cosine':
        v = cf / (np.sqrt(ni) * np.sqrt(nj))
    elif sim == 'jaccard':
        v = cf / (ni + nj - cf)
    elif sim == 'asymmetric_cosine':
        v = cf / (np.power(ni, alpha) * np.power(nj, 1 - alpha))
    elif sim == 'sorensen_dice':
        v = 2 * cf / (ni + nj)
    elif sim == 'tversky':
        v = cf / (cf + alpha * (ni - cf) + beta * (nj - cf))
    else:
        raise ValueError(sim)
    return v * (cf / (cf + shrinkage))


def _roundings(ni, nj, sim, shrinkage, alpha):
    """elementwise N of (b)"""
    rounds = {'cosine': 4., 'jaccard': 1., 'sorensen_dice': 1., 'tversky': 5.}.get(sim)
    if sim == 'asymmetric_cosine':
        rounds = 2. + 2 * POWF_U + alpha * np.log(np.maximum(ni, 1.)) + (alpha + abs(1 - alpha)) * np.log(np.maximum(nj, 1.))
    return rounds + (4. if shrinkage > 0 else 0.)


def values(x, sim, shrinkage=0., alpha=None, beta=None, c=None):
    """float64 [n, n]: the similarity of every candidate pair, 0 elsewhere (no common feature, the diagonal)"""
    c = counts(x) if c is None else c
    n = np.diag(c).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        v = _formula(c.astype(np.float64), n[:, None], n[None, :], sim, shrinkage, alpha, beta)
    v[c == 0] = 0.
    np.fill_diagonal(v, 0.)
    return v


def value_bound(x, sim, shrinkage=0., alpha=None, beta=None, c=None, v=None):
    """float64 [n, n]: bound of |fp32 kernel value - values()| per pair, (b) above"""
    c = counts(x) if c is None else c
    v = values(x, sim, shrinkage, alpha, beta, c) if v is None else v
    n = np.diag(c).astype(np.float64)
    return v * gamma(_roundings(n[:, None], n[None, :], sim, shrinkage, alpha) + np.zeros_like(v))


def sparse_values_and_bound(x, sim, shrinkage=0., alpha=None, beta=None):
    """values() and value_bound() of a large sparse 0/1 matrix as two CSR matrices of one structure (the candidate pairs, columns ascending)"""
    x = sp.csr_matrix((np.ones(x.nnz, dtype=np.int64), x.nonzero()), shape=x.shape)
    n = np.asarray(x.sum(axis=1)).ravel().astype(np.float64)
    c = sp.coo_matrix(x @ x.T)
    keep = (c.row != c.col) & (c.data > 0)
    row, col, cf = c.row[keep], c.col[keep], c.data[keep].astype(np.float64)
    v = _formula(cf, n[row], n[col], sim, shrinkage, alpha, beta)
    b = v * gamma(_roundings(n[row], n[col], sim, shrinkage, alpha) + np.zeros_like(v))
    out = []
    for d in (v, b):
        m = sp.csr_matrix((d, (row, col)), shape=c.shape)
        m.sort_indices()
        out.append(m)
    return out[0], out[1]


def check_kernel_lists(idx, val, length, v, b, k, rows=None, what=''):
    """The per-row rule of the kernel tests. idx / val / length: the kernel's lists (numpy); v, b: CSR matrices of the float64 values
    and their bounds (structure = the candidates). Per row: sorted by (returned value descending, index ascending); no self, no
    duplicate, no index with count 0; length = min(k, candidates); |val - v[idx]| <= bound; no candidate outside the list has a
    float64 value above the list's smallest by more than the two bounds involved (the kernel ranks fp32 values: value_out - bound_out
    <= value_in + bound_in); (-1, 0) behind the length."""
    v, b = sp.csr_matrix(v), sp.csr_matrix(b)
    for i in (range(v.shape[0]) if rows is None else rows):
        cand, cv, cb = v.indices[v.indptr[i]:v.indptr[i + 1]], v.data[v.indptr[i]:v.indptr[i + 1]], b.data[b.indptr[i]:b.indptr[i + 1]]
        n_l = int(length[i])
        assert n_l == min(k, len(cand)), f'{what} row {i}: length {n_l}, {len(cand)} candidates, k = {k}'
        assert np.all(idx[i, n_l:] == -1) and np.all(val[i, n_l:].view(np.int32) == 0), f'{what} row {i}: padding is not (-1, +0)'
        if n_l == 0:
            continue
        g, gv = idx[i, :n_l].astype(np.int64), val[i, :n_l]
        pos = np.searchsorted(cand, g)
        assert np.all(pos < len(cand)) and np.all(cand[np.minimum(pos, len(cand) - 1)] == g), f'{what} row {i}: a neighbour without a common feature (or self)'
        assert len(np.unique(g)) == n_l, f'{what} row {i}: duplicate neighbour'
        assert np.all((gv[:-1] > gv[1:]) | ((gv[:-1] == gv[1:]) & (g[:-1] < g[1:]))), f'{what} row {i}: not sorted by (value desc, index asc)'
        err = np.abs(gv.astype(np.float64) - cv[pos])
        assert np.all(err <= cb[pos]), f'{what} row {i}: value error {err.max():.3e} over its bound {cb[pos][err.argmax()]:.3e}'
        if n_l < len(cand):
            out = np.ones(len(cand), dtype=bool)
            out[pos] = False
            weakest = np.argmin(cv[pos])
            assert np.all(cv[out] - cb[out] <= cv[pos][weakest] + cb[pos][weakest]), f'{what} row {i}: a better candidate was left out'


def lists(v, k):
    """the canonical lists of a value matrix: idx int64 [n, k] (-1 behind the length), val float64 [n, k] (0 there), len int64 [n]"""
    n = v.shape[0]
    idx, val, length = np.full((n, k), -1, dtype=np.int64), np.zeros((n, k)), np.zeros(n, dtype=np.int64)
    for i in range(n):
        cand = np.flatnonzero(v[i] > 0)
        order = cand[np.lexsort((cand, -v[i, cand]))][:k]
        length[i] = len(order)
        idx[i, :len(order)], val[i, :len(order)] = order, v[i, order]
    return idx, val, length


def lists_to_dense(idx, val, length):
    """S [n, n] float64 of a set of lists"""
    n = idx.shape[0]
    s = np.zeros((n, n))
    for i in range(n):
        s[i, idx[i, :length[i]]] = val[i, :length[i]]
    return s


def predict(alg, s, x):
    """dense float64 [users, items]: 'uknn' S X (knn_algs.py:96), 'iknn' X S^T (knn_algs.py:116); x = the user x item 0/1 matrix"""
    x = dense01(x).astype(np.float64)
    return s @ x if alg == 'uknn' else x @ s.T


def csr_rows_times_csr_ordered(x, rows, y):
    """float32 [len(rows), y.shape[1]]: the order oracle of sbr_csr_rows_times_csr. A cell's float32 accumulator receives x[p] * y[col(p), c]
    over the entries p of X's row in ascending column of X, one np.float32 addition each (a cell without an entry of Y's row receives
    nothing). Equal in bits to the kernel's acc = fmaf(x, y, acc) when every product is exact in float32: fmaf then is the exact product
    followed by one rounded addition. ordered_product_operands() gives such operands (X holds powers of two)."""
    x, y = sp.csr_matrix(x), sp.csr_matrix(y)
    assert x.has_sorted_indices and y.has_sorted_indices and x.dtype == y.dtype == np.float32
    out = np.zeros((len(rows), y.shape[1]), dtype=np.float32)
    for b, r in enumerate(rows):
        for p in range(x.indptr[r], x.indptr[r + 1]):
            lo, hi = y.indptr[x.indices[p]], y.indptr[x.indices[p] + 1]
            cols = y.indices[lo:hi]                                            # distinct: one addition per cell
            out[b, cols] = out[b, cols] + x.data[p] * y.data[lo:hi]
    return out


def ordered_product_operands(n_cols):
    """(x, rows, y) for the order pin of sbr_csr_rows_times_csr. X [6, 130]: rows of 0, 1, 63, 64, 65 and 130 entries (the edges of the
    64-entry staging loop) with values 2^-3 ... 2^3, so every product is exact; ``rows`` names them out of order, one twice. Y
    [130, n_cols] float32 in [-4, 4]: rows of 0, 5, 128 and 129 entries in turn (either side of the scan limit of 128; a Y of fewer than
    130 columns has no such rows: 0, 5, n_cols / 2 and n_cols entries then), the 5-entry rows with columns 15 and 16 on the two sides
    of a strip edge."""
    rng = np.random.default_rng(1000 + n_cols)
    x = np.zeros((6, 130), dtype=np.float32)
    for r, cnt in enumerate((0, 1, 63, 64, 65, 130)):
        x[r, rng.choice(130, cnt, replace=False)] = 2.0 ** rng.integers(-3, 4, cnt)
    y = np.zeros((130, n_cols), dtype=np.float32)
    for j in range(130):
        cnt = ((0, 5, 128, 129) if n_cols >= 130 else (0, 5, n_cols // 2, n_cols))[j % 4]
        cols = rng.choice(n_cols, cnt, replace=False)
        if cnt == 5:
            cols = np.concatenate(([15, 16], np.setdiff1d(cols, [15, 16])[:3]))
        y[j, cols] = rng.uniform(0.001, 4., cnt) * rng.choice([-1., 1.], cnt)
    x, y = sp.csr_matrix(x), sp.csr_matrix(y)
    x.sort_indices()
    y.sort_indices()
    return x, np.array([5, 0, 3, 1, 2, 4, 3], dtype=np.int64), y


def entity_matrix(alg, x):
    """the matrix whose rows are compared: users x items for 'uknn', items x users for 'iknn'"""
    x = dense01(x)
    return x if alg == 'uknn' else x.T.copy()


def boundary_tied(v, k):
    """bool [n]: the k-th and (k+1)-th candidate values of the row differ by at most TIE_REL relative (rows with <= k candidates: False)"""
    out = np.zeros(v.shape[0], dtype=bool)
    for i in range(v.shape[0]):
        s = np.sort(v[i][v[i] > 0])[::-1]
        if len(s) > k:
            out[i] = (s[k - 1] - s[k]) <= TIE_REL * s[k - 1]
    return out


# ---- (c): the fixture rule ------------------------------------------------------------------------------------------------------------
def fixture_rows(indptr, indices, data):
    """the reference's sim_mtx rows without their explicit zeros -> list of (indices, values)"""
    rows = []
    for i in range(len(indptr) - 1):
        ind, dat = indices[indptr[i]:indptr[i + 1]], data[indptr[i]:indptr[i + 1]]
        rows.append((ind[dat != 0], dat[dat != 0]))
    return rows


def check_lists_against_fixture(got_idx, got_val, got_len, ref_rows, v64, k, tol, what=''):
    """got_*: lists under test; ref_rows: fixture_rows of the case; v64: values() of the case's entity matrix; tol [n, n]: allowed
    |got value - reference value| per pair. Returns the number of rows whose index sets were compared."""
    n = len(ref_rows)
    tied = boundary_tied(v64, k)
    compared = 0
    for i in range(n):
        r_ind, r_val = ref_rows[i]
        g_ind, g_val = np.asarray(got_idx[i, :got_len[i]]), np.asarray(got_val[i, :got_len[i]], dtype=np.float64)
        assert len(g_ind) == len(r_ind), f'{what} row {i}: {len(g_ind)} neighbours, the reference has {len(r_ind)}'
        assert len(set(g_ind.tolist())) == len(g_ind) and i not in g_ind, f'{what} row {i}: duplicate neighbour or self'
        t = tol[i, g_ind]
        assert np.all(np.abs(g_val - v64[i, g_ind]) <= t), f'{what} row {i}: a value differs from the float64 value of its own index'
        rs, gs = np.sort(r_val)[::-1], np.sort(g_val)[::-1]
        # sorting moves a value by no more than the largest error of the row; 1e-12: the reference's own float64 operation order
        assert np.all(np.abs(rs - gs) <= t.max(initial=0.) + 1e-12 * rs), f'{what} row {i}: sorted values differ from the reference'
        if not tied[i]:
            compared += 1
            assert set(g_ind.tolist()) == set(r_ind.tolist()), f'{what} row {i}: neighbour set differs from the reference'
    return compared


def gamma(t):
    """gamma_t = t u / (1 - t u): the bound of a sum of t fp32 terms added one after the other"""
    t = np.asarray(t, dtype=np.float64)
    return t * U32 / (1 - t * U32)


def load_g22():
    """(arrays, cases) of tests/golden/g22_knn.{npz,json}"""
    import json
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    with np.load(os.path.join(here, 'g22_knn.npz')) as f:
        arrays = {k: f[k] for k in f.files}
    return arrays, json.load(open(os.path.join(here, 'g22_knn.json')))['cases']


def check_case_against_fixture(case, arrays, got_idx, got_val, got_len, got_pred, tol_of, what=''):
    """The whole rule (c) for one g22 case. got_*: lists and dense score matrix [users, items] under test; tol_of(v64, c) -> the allowed
    value error per pair [n, n]. pred_mtx is compared at k = 60 with the bound of its sum: the value errors of the terms plus
    gamma_t of the fp32 summation when the values are fp32 (tol > 0), nothing when they are float64."""
    x = arrays['inter']
    ent = entity_matrix(case['alg'], x)
    c = counts(ent)
    v64 = values(ent, case['sim'], case['shrinkage'], case['params'].get('alpha'), case['params'].get('beta'), c)
    tol = tol_of(v64, c)
    name = case['name']
    ref_rows = fixture_rows(arrays[f'{name}/sim/indptr'], arrays[f'{name}/sim/indices'], arrays[f'{name}/sim/data'])
    compared = check_lists_against_fixture(got_idx, got_val, got_len, ref_rows, v64, case['k'], tol, what or name)
    assert compared == case['rows'] - case['rows_tied_at_boundary'], f'{name}: {compared} rows compared by index set'
    if case['k'] == 60:
        ref_pred = arrays[f'{name}/pred_mtx']
        s_tol = np.where(v64 > 0, tol, 0.)
        terms = predict(case['alg'], v64, x)                                   # all terms are >= 0: the sum of their magnitudes
        n_terms = predict(case['alg'], (v64 > 0).astype(np.float64), x)
        bound = predict(case['alg'], s_tol, x) + (gamma(n_terms) * terms if tol.max() > 0 else 0.) + 1e-12 * np.abs(ref_pred)
        err = np.abs(np.asarray(got_pred, dtype=np.float64) - ref_pred)
        assert np.all(err <= bound), f'{name}: pred_mtx differs from the reference, worst {err.max():.3e} over its bound at {np.unravel_index((err - bound).argmax(), err.shape)}'
    return compared
