"""Float64 restatement of ItemFeatureKNN (csrc/dense_knn.hip; utilities/similarities.py:18-61, :86-93, algorithms/knn_algs.py:121-140), the
fp32 error bound of a similarity value and the comparison rules of the kernel tests and of the g25 fixture. A plain module: no fixtures, no
pytest hooks, no GPU. tests/test_ifknn_cpu.py shows that the restatement meets the fixture recorded from the reference;
tests/test_hip_ifknn.py applies restatement, bound and rules to the kernel and the model.

(a) Restatement. F [n, d]; dot = F F^T, norm_i = sqrt(dot_ii). j is a candidate of i iff dot_ij != 0 (scipy's coo_matrix drops the exact
zeros of the dense product), j = i included when the row is not zero. For j != i: v = dot / (norm_i norm_j), value = v dot / (dot + shrinkage)
(shrinkage = 0: v); value_ii = 0. The list of row i: its candidates by np.lexsort (value descending, index ascending), cut at k — the
project's canonical rule; a row with fewer than k positive values keeps its self 0 and then negative values. The reference cuts with an
unstable argsort; see (d). Prediction: M S^T with S the matrix of the lists (M: users x items).

(b) Bound — derived from the kernel's operation order (include/sibrar_hip.h), never fitted. u = 2^-24, one fp32 operation returns
x (1 + e), |e| <= u; gamma_t = t u / (1 - t u). The inputs are fp32 numbers, exact in float64. With S_ij = sum_k |x_k y_k|:
    dot    a chain of d fmaf:                      |fl(dot) - dot| <= D = gamma_d S_ij
    q_i    the same chain, all terms >= 0:         relative g = gamma_d;  sqrtf: norm relative  e_n = (1 + g/2 + g^2/2)(1 + u) - 1
    den    norm_i * norm_j, one rounding:          relative e_d = (1 + e_n)^2 (1 + u) - 1
    v      fl(dot) / fl(den), one rounding:        |fl(v) - v| <= b_v = |v| (A - 1) + (D / den) A,   A = (1 + u) / (1 - e_d)
  two roundings after the dot for shrinkage = 0. shrinkage > 0 (stated for dot >= 0 only: features >= 0, the model's restriction):
    t      fl(dot) + fl(shrinkage), one rounding:  |fl(t) - t| <= E = (D + u shrinkage)(1 + u) + u t
    s      fl(dot) / fl(t), one rounding:          |fl(s) - s| <= b_s = s (B - 1) + (D / t) B,       B = (1 + u) / (1 - E / t)
    value  fl(v) * fl(s), one rounding:            |fl(value) - value| <= (b_v (s + b_s) + |v| b_s)(1 + u) + u |v s|
  five roundings after the dot. The self entry is exactly +0.

(c) The kernel's list rule: check_kernel_lists below. (d) The fixture rule, as tests/knn_ref.py (c) with the explicit zeros kept:
    k = 60   nothing is pruned in the 40-item world: sim_mtx (the self 0 included) and the dense pred_mtx are compared in full;
    k = 5    the sorted values of every row are compared, and the index sets of the rows whose 5th and 6th candidate values differ by
             more than 1e-6 relative."""
import json
import os

import numpy as np

U32 = 2.0 ** -24
TIE_REL = 1e-6


def gamma(t):
    t = np.asarray(t, dtype=np.float64)
    return t * U32 / (1 - t * U32)


def dots(f):
    """(dot [n, n], S [n, n] = sum_k |x_k y_k|, norms [n]) in float64"""
    f = np.asarray(f, dtype=np.float64)
    dot = f @ f.T
    return dot, np.abs(f) @ np.abs(f).T, np.sqrt(np.einsum('ik,ik->i', f, f))


def values(f, shrinkage=0.):
    """(value float64 [n, n], candidates bool [n, n]) of (a); value is 0 outside the candidates and on the diagonal"""
    dot, _, nrm = dots(f)
    cand = dot != 0
    with np.errstate(divide='ignore', invalid='ignore'):
        v = dot / (nrm[:, None] * nrm[None, :])
        if shrinkage > 0:
            v = v * (dot / (dot + shrinkage))
    v[~cand] = 0.
    np.fill_diagonal(v, 0.)
    return v, cand


def value_bound(f, shrinkage=0.):
    """float64 [n, n]: bound of |fp32 kernel value - values()| per pair, (b) above; f: the fp32 features the kernel is given"""
    f = np.asarray(f)
    assert f.dtype == np.float32
    d = f.shape[1]
    dot, s_abs, nrm = dots(f)
    v, cand = values(f, shrinkage)
    if shrinkage > 0:
        assert (dot >= 0).all(), 'the bound with shrinkage is stated for dot >= 0 only'
        v_plain = values(f, 0.)[0]
    else:
        v_plain = v
    g = float(gamma(d))
    e_n = (1 + g / 2 + g * g / 2) * (1 + U32) - 1
    e_d = (1 + e_n) ** 2 * (1 + U32) - 1
    a = (1 + U32) / (1 - e_d)
    big_d = g * s_abs
    with np.errstate(divide='ignore', invalid='ignore'):
        den = nrm[:, None] * nrm[None, :]
        b_v = np.abs(v_plain) * (a - 1) + big_d / den * a
        b = b_v
        if shrinkage > 0:
            t = dot + shrinkage
            s = dot / t
            e_t = (big_d + U32 * shrinkage) * (1 + U32) + U32 * t
            bb = (1 + U32) / (1 - e_t / t)
            b_s = s * (bb - 1) + big_d / t * bb
            b = (b_v * (s + b_s) + np.abs(v_plain) * b_s) * (1 + U32) + U32 * np.abs(v_plain * s)
    b = np.where(cand, b, 0.)
    np.fill_diagonal(b, 0.)
    return b


def candidates_are_precision_free(f, rel=1e-9):
    """no pair has a float64 |dot| below rel * sum_k |x_k y_k| other than exact zeros: every precision names the same candidates"""
    dot, s_abs, _ = dots(f)
    return not bool(((dot != 0) & (np.abs(dot) < rel * s_abs)).any())


def lists(v, cand, k):
    """the canonical lists of (a): idx int64 [n, k] (-1 behind the length), val float64 [n, k] (0 there), len int64 [n]"""
    n = v.shape[0]
    idx, val, length = np.full((n, k), -1, dtype=np.int64), np.zeros((n, k)), np.zeros(n, dtype=np.int64)
    for i in range(n):
        c = np.flatnonzero(cand[i])
        order = c[np.lexsort((c, -v[i, c]))][:k]
        length[i] = len(order)
        idx[i, :len(order)], val[i, :len(order)] = order, v[i, order]
    return idx, val, length


def lists_to_dense(idx, val, length):
    n = idx.shape[0]
    s = np.zeros((n, n))
    for i in range(n):
        s[i, idx[i, :length[i]]] = val[i, :length[i]]
    return s


def predict(s, x):
    """dense float64 [users, items]: X S^T (knn_algs.py:138); x = the user x item 0/1 matrix"""
    return (np.asarray(x) != 0).astype(np.float64) @ s.T


def boundary_tied(v, cand, k):
    """bool [n]: the k-th and (k+1)-th candidate values of the row differ by at most TIE_REL relative (rows with <= k candidates: False)"""
    out = np.zeros(v.shape[0], dtype=bool)
    for i in range(v.shape[0]):
        s = np.sort(v[i][cand[i]])[::-1]
        if len(s) > k:
            out[i] = (s[k - 1] - s[k]) <= TIE_REL * abs(s[k - 1])
    return out


# ---- (c): the kernel's list rule ---------------------------------------------------------------------------------------------------------
def check_kernel_lists(idx, val, length, v, cand, b, k, rows=None, what=''):
    """idx / val / length: the kernel's lists (numpy); v, cand, b: values(), candidates and value_bound(). Per row: sorted by (returned
    value descending, index ascending); every index a candidate, none twice; the self entry, where listed, has the value +0 exactly;
    length = min(k, candidates); |val - v[idx]| <= bound; no candidate outside the list has a float64 value above the list's smallest by
    more than the two bounds involved (value_out - bound_out <= value_in + bound_in); (-1, +0) behind the length."""
    for i in (range(v.shape[0]) if rows is None else rows):
        c = np.flatnonzero(cand[i])
        n_l = int(length[i])
        assert n_l == min(k, len(c)), f'{what} row {i}: length {n_l}, {len(c)} candidates, k = {k}'
        assert np.all(idx[i, n_l:] == -1) and np.all(val[i, n_l:].view(np.int32) == 0), f'{what} row {i}: padding is not (-1, +0)'
        if n_l == 0:
            continue
        g, gv = idx[i, :n_l].astype(np.int64), val[i, :n_l]
        assert np.all((g >= 0) & (g < v.shape[0])) and np.all(cand[i, g]), f'{what} row {i}: a neighbour that is no candidate'
        assert len(np.unique(g)) == n_l, f'{what} row {i}: duplicate neighbour'
        assert np.all(gv[g == i].view(np.int32) == 0), f'{what} row {i}: the self entry is not +0'
        assert not np.any((gv == 0) & (gv.view(np.int32) != 0)), f'{what} row {i}: a -0 value'
        assert np.all((gv[:-1] > gv[1:]) | ((gv[:-1] == gv[1:]) & (g[:-1] < g[1:]))), f'{what} row {i}: not sorted by (value desc, index asc)'
        err = np.abs(gv.astype(np.float64) - v[i, g])
        assert np.all(err <= b[i, g]), f'{what} row {i}: value error {err.max():.3e} over its bound {b[i, g][err.argmax()]:.3e}'
        if n_l < len(c):
            out = np.setdiff1d(c, g)
            weakest = g[np.argmin(v[i, g])]
            assert np.all(v[i, out] - b[i, out] <= v[i, weakest] + b[i, weakest]), f'{what} row {i}: a better candidate was left out'


# ---- (d): the fixture rule ---------------------------------------------------------------------------------------------------------------
def fixture_rows(indptr, indices, data):
    """the reference's sim_mtx rows, explicit zeros kept -> list of (indices, values)"""
    return [(indices[indptr[i]:indptr[i + 1]], data[indptr[i]:indptr[i + 1]]) for i in range(len(indptr) - 1)]


def check_lists_against_fixture(got_idx, got_val, got_len, ref_rows, v64, cand, k, tol, what=''):
    """got_*: lists under test; ref_rows: fixture_rows of the case; v64, cand: values() of the case's features; tol [n, n]: allowed
    |got value - reference value| per pair. Returns the number of rows whose index sets were compared."""
    tied = boundary_tied(v64, cand, k)
    compared = 0
    for i, (r_ind, r_val) in enumerate(ref_rows):
        g_ind, g_val = np.asarray(got_idx[i, :got_len[i]]), np.asarray(got_val[i, :got_len[i]], dtype=np.float64)
        assert len(g_ind) == len(r_ind), f'{what} row {i}: {len(g_ind)} neighbours, the reference has {len(r_ind)}'
        assert len(set(g_ind.tolist())) == len(g_ind), f'{what} row {i}: duplicate neighbour'
        assert np.all(cand[i, g_ind]), f'{what} row {i}: a neighbour that is no candidate'
        assert np.all(g_val[g_ind == i] == 0), f'{what} row {i}: the self entry is not 0'
        t = tol[i, g_ind]
        assert np.all(np.abs(g_val - v64[i, g_ind]) <= t), f'{what} row {i}: a value differs from the float64 value of its own index'
        rs, gs = np.sort(r_val)[::-1], np.sort(g_val)[::-1]
        # sorting moves a value by no more than the largest error of the row; 1e-12: the reference's own float64 operation order
        assert np.all(np.abs(rs - gs) <= t.max(initial=0.) + 1e-12 * np.abs(rs)), f'{what} row {i}: sorted values differ from the reference'
        if not tied[i]:
            compared += 1
            assert set(g_ind.tolist()) == set(r_ind.tolist()), f'{what} row {i}: neighbour set differs from the reference'
    return compared


def load_g25():
    """(arrays, cases) of tests/golden/g25_ifknn.{npz,json}"""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    with np.load(os.path.join(here, 'g25_ifknn.npz')) as f:
        arrays = {k: f[k] for k in f.files}
    return arrays, json.load(open(os.path.join(here, 'g25_ifknn.json')))['cases']


def case_features(case, arrays):
    """the case's feature matrix, float64 [n_items, d]"""
    return np.abs(arrays['features']) if case['features'] == 'abs' else arrays['features']


def check_case_against_fixture(case, arrays, got_idx, got_val, got_len, got_pred, fp32, what=''):
    """The whole rule (d) for one g25 case. got_*: lists and dense score matrix [users, items] under test. fp32: the values under test
    are the kernel's (tolerance: value_bound of the features rounded to fp32, plus what that rounding moves the float64 value by — the
    fixture's features are float64) or float64 (tolerance 1e-12 relative). pred_mtx is compared at k = 60 with the bound of its sum: the
    value errors of the terms plus gamma_t of the fp32 fmaf summation."""
    x, f64 = arrays['inter'], case_features(case, arrays)
    v64, cand = values(f64, case['shrinkage'])
    if fp32:
        f32 = f64.astype(np.float32)
        v32, cand32 = values(f32, case['shrinkage'])
        assert np.array_equal(cand, cand32)
        tol = value_bound(f32, case['shrinkage']) + np.abs(v32 - v64)
    else:
        tol = 1e-12 * np.abs(v64)
    name = case['name']
    ref_rows = fixture_rows(arrays[f'{name}/sim/indptr'], arrays[f'{name}/sim/indices'], arrays[f'{name}/sim/data'])
    compared = check_lists_against_fixture(got_idx, got_val, got_len, ref_rows, v64, cand, case['k'], tol, what or name)
    assert compared == case['rows'] - case['rows_tied_at_boundary'], f'{name}: {compared} rows compared by index set'
    if case['k'] == 60:
        ref_pred = arrays[f'{name}/pred_mtx']
        s_tol = predict(np.where(cand, tol, 0.), x)
        terms = predict(np.abs(v64), x) + s_tol
        bound = s_tol + (gamma(predict(cand.astype(np.float64), x)) * terms if fp32 else 0.) + 1e-12 * np.abs(ref_pred)
        err = np.abs(np.asarray(got_pred, dtype=np.float64) - ref_pred)
        assert np.all(err <= bound), f'{name}: pred_mtx differs from the reference, worst {err.max():.3e} over its bound at {np.unravel_index((err - bound).argmax(), err.shape)}'
    return compared


# ---- the numpy float32 restatement of the header's operation order, for operands whose dots are exact (small integers) ------------------
def lists_f32_exact(f, k, shrinkage=0.):
    """(idx int32 [n, k], val float32 [n, k], len int32 [n]) as the kernel must give them bit for bit when every product and partial sum
    of the dots is exact in fp32 (asserted: integer features with d max|x|^2 < 2^24), so that the fmaf chains are order-free: norms by
    np.sqrt on float32 (correctly rounded), then *, / (and +, /, * with shrinkage) as single float32 operations."""
    f = np.asarray(f, dtype=np.float32)
    assert np.all(f == np.round(f)) and f.shape[1] * float(np.abs(f).max(initial=0.)) ** 2 < 2 ** 24
    n = f.shape[0]
    dot = (f.astype(np.float64) @ f.astype(np.float64).T).astype(np.float32)
    nrm = np.sqrt(np.diag(dot))
    shr = np.float32(shrinkage)
    with np.errstate(divide='ignore', invalid='ignore'):
        val = dot / (nrm[:, None] * nrm[None, :])
        if shrinkage > 0:
            val = val * (dot / (dot + shr))
    assert val.dtype == np.float32
    cand = dot != 0
    val[~cand] = 0.
    np.fill_diagonal(val, 0.)
    val = val + np.float32(0.)                       # -0 -> +0
    idx, out, length = np.full((n, k), -1, dtype=np.int32), np.zeros((n, k), dtype=np.float32), np.zeros(n, dtype=np.int32)
    for i in range(n):
        c = np.flatnonzero(cand[i])
        order = c[np.lexsort((c, -val[i, c]))][:k]
        length[i] = len(order)
        idx[i, :len(order)], out[i, :len(order)] = order, val[i, order]
    return idx, out, length
