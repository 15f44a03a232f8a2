"""RBMF (algorithms/mf_algs.py:145-211) in numpy. ``maxvolpy`` is not available, so there is no recorded fixture: maxvol is restated here
from the published algorithm (Goreinov, Oseledets, Savostyanov, Tyrtyshnikov and Zamarashkin 2010) as sibrar_amd.ops.maxvol runs it.
The ORACLE is the float64 run (``dtype=np.float64``); the same functions in float32 are the YARDSTICK whose excess over ``tol`` and
whose error in the ridge solve the kernels may exceed by a stated factor. Every arg-max (largest magnitude, then the lowest row, then the
lowest column) also reports the ratio runner-up / winner, and the final comparison with ``tol`` its own ratio: where the worst of them
is close to 1 a float32 run may legitimately decide differently, and the tests that compare decisions assert that it is not.
A plain module: no fixtures, no pytest hooks."""
import numpy as np
import scipy.sparse as sp

from svd_ref import canonical, planted                      # noqa: F401  (the planted block worlds)

EPS = 2.0 ** -24                      # unit roundoff of fp32
TOL = 1.05                            # maxvolpy's defaults, as remembered
MAX_ITERS = 100
RATIO_MAX = 1 - 1e-4                  # decisions are compared only where every runner-up / winner ratio is at most this
MODEL_FACTOR = 10                     # kernel figures <= 10 x the float32 restatement's (the margin of svd_ref.MODEL_FACTOR)

#         users, items, groups, p_in, p_out, seed, r
WORLDS = {'700x257/r24': (700, 257, 12, 0.5, 0.04, 4, 24), '129x130/r64': (129, 130, 6, 0.6, 0.05, 2, 64),
          '1000x400/r100': (1000, 400, 20, 0.5, 0.03, 7, 100)}


def gamma(k):
    """Higham's gamma_k for fp32"""
    return k * EPS / (1 - k * EPS)


def _ratio(mags):
    """runner-up / winner of a vector of magnitudes (0 when there is no runner-up or the winner is 0)"""
    if mags.size < 2:
        return 0.0
    top = np.partition(mags, -2)[-2:]
    return float(top[0] / top[1]) if top[1] > 0 else 0.0


def lu_pivots(u, dtype=np.float64):
    """the row-pivoted LU of sbr_maxvol_lu_step_f32 -> (idx [r], L [n, r] unit lower over all rows, Ltop [r, r], Utop [r, r], ratios)"""
    a = np.array(u, dtype=dtype)
    n, r = a.shape
    free = np.ones(n, dtype=bool)
    pos = np.full(n, -1)
    idx, ratios = [], []
    for k in range(r):
        mag = np.where(free, np.abs(a[:, k]), -1.0)
        p = int(np.argmax(mag))                                    # the lowest row of a tie
        ratios.append(_ratio(mag[free]))
        idx.append(p)
        free[p], pos[p] = False, k
        l = (a[free, k] / a[p, k]).astype(dtype)
        a[free, k] = l
        a[np.ix_(free, np.arange(k + 1, r))] -= np.outer(l, a[p, k + 1:]).astype(dtype)
    idx = np.array(idx)
    utop = np.triu(a[idx])
    L = a.copy()
    for s, p in enumerate(idx):
        L[p, s], L[p, s + 1:] = 1, 0
    return idx, L, L[idx].copy(), utop, ratios


def basis_matrix(u, idx, dtype=np.float64):
    """B = u inv(u[idx]) in ``dtype`` (a solve, no inverse)"""
    u = np.asarray(u, dtype=dtype)
    return np.linalg.solve(u[idx].T, u.T).T.astype(dtype)


def certificate(u, idx):
    """max |u inv(u[idx])| in float64: what maxvol promises to bring to <= tol"""
    return float(np.abs(basis_matrix(u, idx, np.float64)).max())


def maxvol(u, tol=TOL, max_iters=MAX_ITERS, dtype=np.float64, start=None):
    """-> (idx [r] in basis order, n_swaps, worst decision ratio). ``start``: the initial rows instead of the LU's pivots"""
    u = np.asarray(u, dtype=dtype)
    n, r = u.shape
    if start is None:
        idx, _, _, _, ratios = lu_pivots(u, dtype)
    else:
        idx, ratios = np.array(start), []
    idx = idx.copy()
    B = basis_matrix(u, idx, dtype)
    B[idx] = np.eye(r, dtype=dtype)
    swaps = 0
    while True:
        mag = np.abs(B)
        flat = int(np.argmax(mag))                                 # row-major: the lowest row, then the lowest column of a tie
        i, j = divmod(flat, r)
        top = float(mag[i, j])
        ratios.append(min(top, tol) / max(top, tol))               # the comparison with tol is a decision too
        if not top > tol or swaps >= max_iters:
            break
        ratios.append(_ratio(mag.ravel()))
        w = ((B[i] - np.eye(r, dtype=dtype)[j]) / B[i, j]).astype(dtype)
        B = (B - np.outer(B[:, j], w)).astype(dtype)
        B[i] = np.eye(r, dtype=dtype)[j]
        idx[j] = i
        swaps += 1
    return idx, swaps, max(ratios)


def ridge(x, idx, lam, dtype=np.float64, literal=False):
    """the closed form of mf_algs.py:178-184 from the representatives ``idx`` -> (X [n_users, r], C [n_items, r]) in ``dtype``.
    ``literal``: as the reference writes it, ``matrix @ C.T @ inv(C @ C.T + lam I)`` with an explicit inverse — in float32 the
    YARDSTICK of the model's X; otherwise one LAPACK solve — in float64 the ORACLE. (In float32 the LU solve is no fair yardstick: on the
    representatives' own rows the right-hand side is a column of the factored matrix, which the substitution reproduces without any
    rounding, and those rows hold the largest elements of X; LAPACK's own float32 Cholesky solve errs 4 to 11 times as much.)"""
    x = canonical(x).astype(dtype)
    C = np.asarray(x[np.asarray(idx)].todense(), dtype=dtype)      # [r, n_items]
    K = (C @ C.T + dtype(lam) * np.eye(len(idx), dtype=dtype)).astype(dtype)
    M = np.asarray(x @ C.T, dtype=dtype)
    if literal:
        return (M @ np.linalg.inv(K).astype(dtype)).astype(dtype), C.T.copy()
    return np.linalg.solve(K, M.T).T.astype(dtype), C.T.copy()


def tall(n, r, seed):
    """a tall float32 block with orthonormal columns, like a block of singular vectors"""
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, r)))
    return np.ascontiguousarray(q, dtype=np.float32)


def lu_input(n, r):
    """the first seeded ``tall`` block whose float64 LU takes every pivot decision with a ratio <= 1 - 1e-3 -> (u, idx, L, Ltop, Utop,
    worst ratio): the inputs are chosen by the oracle's margins, never by the code under test"""
    for seed in range(200):
        u = tall(n, r, 1000 * r + n + 7919 * seed)
        idx, L, ltop, utop, ratios = lu_pivots(u)
        if max(ratios) <= 1 - 1e-3:
            return u, idx, L, ltop, utop, max(ratios)
    raise AssertionError(f'no input with clear pivots at n={n}, r={r}')


def poor_start_input(n, r, tol=TOL, max_iters=4 * 128):
    """a ``tall`` block whose first r rows are scaled down to 5 %, so that the start ``range(r)`` is poor and the dominant rows lie
    elsewhere; the first seed whose float64 and float32 swap loops from that start both decide with ratios <= 1 - 1e-3 ->
    (u, idx64, swaps64, idx32, swaps32, worst ratio of the float64 run)"""
    for seed in range(200):
        u = tall(n, r, 500 * r + n + 104729 * seed)
        u[:r] *= np.float32(0.05)
        i64, s64, ratio = maxvol(u, tol, max_iters, np.float64, start=np.arange(r))
        if ratio > 1 - 1e-3:
            continue
        i32, s32, _ = maxvol(u, tol, max_iters, np.float32, start=np.arange(r))
        return u, i64, s64, i32, s32, ratio
    raise AssertionError(f'no input with clear decisions at n={n}, r={r}')


def slack(u, idx32, r, tol=TOL):
    """the certificate's allowance over tol: 10 x the float32 restatement's own excess, at least r * 2^-23"""
    return max(MODEL_FACTOR * max(certificate(u, idx32) - tol, 0.0), r * 2.0 ** -23)
