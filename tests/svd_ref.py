"""The truncated SVD of sibrar_amd.svd in numpy. ``svd64`` is the ORACLE: the dense float64 ``numpy.linalg.svd``, which is what the
reference's ``scipy.sparse.linalg.svds`` (algorithms/mf_algs.py:36) converges to; the reference module itself imports ``implicit``, which
is not available, so there is no recorded fixture. ``fit32`` is the YARDSTICK: the block iteration of csrc/svd.hip restated in float32
numpy with LAPACK's float32 ``eigh`` as the eigensolver: the kernels may err a small multiple of what it errs from the same start.
``jacobi32`` restates the pair ordering, the rotation and the stopping rule of ``sbr_sym_eig_f32`` in numpy (float64 arithmetic on the
float32 input, float32 results; every pair of a step at once), so that the algorithm can be checked without a GPU. The worlds are planted block matrices whose spectrum has a gap behind the
number of groups. A plain module: no fixtures, no pytest hooks."""
import numpy as np
import scipy.sparse as sp

EPS = 2.0 ** -24                      # unit roundoff of fp32
EIG_FACTOR = 8                        # eigensolver figures <= 8 x LAPACK's float32 figures (+ n * EPS where those are exactly zero)
MODEL_FACTOR = 10                     # fitted figures <= 10 x the yardstick's: another summation order, an error of the same size
MAX_SWEEPS = 30                       # the sweep cap of sbr_sym_eig_f32
ROTATE_EPS = 2.0 ** -40               # a pair is left alone when |a_pq| <= 2^-40 sqrt(|a_pp| |a_qq|)
TINY_REL = 2.0 ** -46                 # s = sqrt(max(lam, max(lam_0 * 2^-46, FLT_MIN)))

#         users, items, groups, p_in, p_out, seed
WORLDS = {'130x90/g5': (130, 90, 5, 0.6, 0.05, 2), '300x200/g8': (300, 200, 8, 0.6, 0.05, 1), '700x260/g16': (700, 260, 16, 0.5, 0.03, 3)}
GAPLESS = (400, 1000, 100, 0.7, 0.01, 5)


def canonical(m) -> sp.csr_matrix:
    m = sp.csr_matrix(m).copy()
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    return m


def planted(n_users, n_items, g, p_in, p_out, seed) -> sp.csr_matrix:
    """users and items drawn into ``g`` groups; an entry is 1 with probability ``p_in`` inside a block, ``p_out`` outside"""
    rng = np.random.RandomState(seed)
    ug, ig = rng.randint(0, g, size=n_users), rng.randint(0, g, size=n_items)
    p = np.where(ug[:, None] == ig[None, :], p_in, p_out)
    return canonical(sp.csr_matrix((rng.random_sample((n_users, n_items)) < p).astype(np.float64)))


def svd64(x):
    """(u [n, r], s [r] descending, vt [r, m]) of the dense float64 matrix"""
    return np.linalg.svd(np.asarray(sp.csr_matrix(x).todense(), dtype=np.float64), full_matrices=False)


def truncated64(x, k):
    """the best rank-k approximation, float64 [n, m]"""
    u, s, vt = svd64(x)
    return (u[:, :k] * s[:k]) @ vt[:k]


def fix_signs(w):
    """every column's component of largest magnitude (the lowest index on a tie) made positive"""
    at = np.abs(w).argmax(axis=0)
    return w * np.where(w[at, np.arange(w.shape[1])] < 0, -1, 1).astype(w.dtype)


def eigh32(g):
    """LAPACK's float32 eigh, descending, signs fixed -> (lam, W)"""
    lam, w = np.linalg.eigh(np.asarray(g, dtype=np.float32))
    assert lam.dtype == np.float32
    return lam[::-1].copy(), fix_signs(w[:, ::-1].copy())


def round_robin(n):
    """the steps of a sweep of sbr_sym_eig_f32: lists of (p, q), p < q, over N = n rounded up to even; index N - 1 stays"""
    N = n + (n & 1)
    steps = []
    for r in range(N - 1):
        pairs = [(r, N - 1)] + [((r + k) % (N - 1), (r - k) % (N - 1)) for k in range(1, N // 2)]
        steps.append([(min(a, b), max(a, b)) for a, b in pairs])
    return steps


def jacobi32(a):
    """-> (lam descending, W, sweeps run, converged), float32: the Jacobi iteration of sbr_sym_eig_f32, which takes a float32 matrix,
    iterates in float64 and rounds its results once; a step's pairs are rotated at once (rows first, then columns; the kernel's 2 x 2
    blocks do the same and mirror the result)"""
    n = a.shape[0]
    N = n + (n & 1)
    A = np.zeros((N, N), dtype=np.float64)
    A[:n, :n] = np.tril(a) + np.tril(a, -1).T
    W = np.eye(N, dtype=np.float64)
    steps = round_robin(n)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        for sweep in range(MAX_SWEEPS):
            rotated = False
            for pairs in steps:
                p, q = np.array([x[0] for x in pairs]), np.array([x[1] for x in pairs])
                app, aqq, apq = A[p, p], A[q, q], A[p, q]
                on = np.abs(apq) > ROTATE_EPS * (np.sqrt(np.abs(app)) * np.sqrt(np.abs(aqq)))
                if not on.any():
                    continue
                rotated = True
                p, q, app, aqq, apq = p[on], q[on], app[on], aqq[on], apq[on]
                tau = (aqq - app) / (2.0 * apq)
                t = np.where(tau >= 0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
                rp, rq = A[p].copy(), A[q].copy()                              # rows: J^T A
                A[p], A[q] = c[:, None] * rp - s[:, None] * rq, s[:, None] * rp + c[:, None] * rq
                cp, cq = A[:, p].copy(), A[:, q].copy()                        # columns: (J^T A) J
                A[:, p], A[:, q] = c * cp - s * cq, s * cp + c * cq
                A[p, p], A[q, q], A[p, q], A[q, p] = app - t * apq, aqq + t * apq, 0, 0
                A = np.tril(A) + np.tril(A, -1).T                              # the kernel's owner writes both halves
                wp, wq = W[:, p].copy(), W[:, q].copy()
                W[:, p], W[:, q] = c * wp - s * wq, s * wp + c * wq
            if not rotated:
                break
    lam = np.diag(A)[:n]
    order = np.argsort(-lam, kind='stable')
    w = W[:n, :n][:, order]
    return lam[order].astype(np.float32), fix_signs((w / np.sqrt((w * w).sum(axis=0))).astype(np.float32)), sweep + 1, not rotated


def eig_figures(a, lam, w):
    """(residual ||A W - W L||_max / ||A||_max, orthogonality ||W^T W - I||_max) in float64 from the fp32 results"""
    a, lam, w = (np.asarray(v, dtype=np.float64) for v in (a, lam, w))
    scale = np.abs(a).max() or 1.0
    return np.abs(a @ w - w * lam).max() / scale, np.abs(w.T @ w - np.eye(len(lam))).max()


def eig_inputs(n):
    """name -> symmetric float32 [n, n]: the cases of tests/test_hip_svd.py"""
    rng = np.random.default_rng(100 + n)
    d = np.sort(rng.uniform(0.5, 3.0, size=n))[::-1].astype(np.float32)
    y = rng.standard_normal((300, n)).astype(np.float32)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    grade = np.logspace(0, -4, n) if n > 1 else np.ones(1)
    core = q @ np.diag(rng.uniform(0.5, 2.0, size=n)) @ q.T                   # well conditioned: D core D is graded over 1e8
    low = rng.standard_normal((max(n // 2, 1), n)).astype(np.float32)
    rep = np.diag(d.astype(np.float64))
    if n >= 3:                                                                 # one repeated eigenvalue pair, rotated out of the axes
        lam = d.astype(np.float64).copy()
        lam[1] = lam[0]
        rep = q @ np.diag(lam) @ q.T
    cases = {'diagonal': np.diag(d), 'diagonal reversed': np.diag(d[::-1]), 'c I': np.float32(1.75) * np.eye(n, dtype=np.float32),
             'repeated pair': rep, 'gram': y.T @ y, 'graded': grade[:, None] * core * grade[None, :], 'rank deficient': low.T @ low}
    out = {}
    for k, v in cases.items():
        v = np.asarray(v, dtype=np.float32)
        out[k] = np.tril(v) + np.tril(v, -1).T
    return out


def orth32(y, eig=eigh32):
    """(Y W diag(1 / s), s, W), float32"""
    y = np.asarray(y, dtype=np.float32)
    lam, w = eig(y.T @ y)
    tiny = max(np.float32(lam[0]) * np.float32(TINY_REL), np.finfo(np.float32).tiny)
    s = np.sqrt(np.maximum(lam, tiny)).astype(np.float32)
    return ((y @ w) * (np.float32(1) / s)).astype(np.float32), s, w


def fit32(x, v0, factors, n_iterations, tol, eig=eigh32):
    """the block iteration from the start ``v0`` [n_items, b] -> (users_factors, items_factors, s[:factors], iterations run, residuals)"""
    x = canonical(x).astype(np.float32)
    xt = canonical(x.T).astype(np.float32)
    f = factors
    v, _, _ = orth32(v0, eig)
    u = s = None
    history = []
    for it in range(n_iterations + 1):
        y = np.asarray(x @ v, dtype=np.float32)
        if it:
            history.append(float(np.sqrt(((y[:, :f] - u[:, :f] * s[:f]) ** 2).sum(axis=0, dtype=np.float32)).max()))
            if history[-1] <= tol * float(s[0]):
                break
        if it == n_iterations:
            break
        u, _, _ = orth32(y, eig)
        v, s, w = orth32(np.asarray(xt @ u, dtype=np.float32), eig)
        u = (u @ w).astype(np.float32)
    if u is None:
        return y[:, :f], v[:, :f], np.sqrt((y[:, :f] ** 2).sum(axis=0)), 0, history
    return u[:, :f] * s[:f], v[:, :f], s[:f], it, history
