"""Implicit-feedback ALS in numpy, written from the closed-form update of Hu, Koren and Volinsky (2008) with the confidence convention
of algorithms/mf_algs.py:69-142 (``implicit``'s): an observed entry has c = alpha * r, every other entry c = 1; the preference is 1 for
observed entries and 0 elsewhere. For row r with observed columns S:

    A_r = (Y^T Y + reg I) + sum_{i in S} (alpha r_i - 1) y_i y_i^T,   b_r = sum_{i in S} alpha r_i y_i,   x_r = A_r^-1 b_r

``half_sweep64`` / ``fit64`` are the float64 restatement the kernels are pinned to (the reference itself wraps the ``implicit`` library,
which is not available, so there is no recorded fixture). ``half_sweep32`` is the same in float32 — sequential accumulation in CSR order,
then ``scipy.linalg.cho_factor`` / ``cho_solve`` in float32 (LAPACK spotrf / spotrs) — and is the YARDSTICK of the tolerances: the kernel
may err a small multiple of what this plain fp32 solve errs on the same inputs. A plain module: no fixtures, no pytest hooks."""
import numpy as np
import scipy.linalg
import scipy.sparse as sp
import torch

EPS = 2.0 ** -24                      # unit roundoff of fp32
BACKWARD_FACTOR = 8                   # kernel backward error <= 8 x the yardstick's: another summation order, an unblocked factorisation
SCORE_FACTOR = 10                     # fitted scores: deviation from float64 <= 10 x the yardstick's


def canonical(m) -> sp.csr_matrix:
    m = sp.csr_matrix(m).copy()
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    return m


def system64(x: sp.csr_matrix, r: int, y, g, alpha):
    """(A_r, b_r) in float64 from the inputs as given (float32 inputs are converted exactly)"""
    y = np.asarray(y, dtype=np.float64)
    cols, vals = x.indices[x.indptr[r]:x.indptr[r + 1]], x.data[x.indptr[r]:x.indptr[r + 1]].astype(np.float64)
    ys = y[cols]
    c = float(alpha) * vals
    return np.asarray(g, dtype=np.float64) + (ys * (c - 1.0)[:, None]).T @ ys, (ys * c[:, None]).sum(axis=0)


def gram64(y, reg):
    y = np.asarray(y, dtype=np.float64)
    return y.T @ y + float(reg) * np.eye(y.shape[1])


def half_sweep64(x: sp.csr_matrix, y, alpha, reg, g=None):
    """every row of the other factor matrix, float64 [n, f]; an empty row is zeros"""
    x = canonical(x)
    g = gram64(y, reg) if g is None else np.asarray(g, dtype=np.float64)
    out = np.zeros((x.shape[0], np.asarray(y).shape[1]))
    for r in range(x.shape[0]):
        if x.indptr[r + 1] > x.indptr[r]:
            a, b = system64(x, r, y, g, alpha)
            out[r] = np.linalg.solve(a, b)
    return out


def fit64(x, users0, items0, alpha, reg, n_iterations, trace=None):
    """n_iterations of (user half-sweep, item half-sweep) from the given initial factors; ``trace``: a list that receives the loss after
    every half-sweep"""
    x = canonical(x)
    xt = canonical(x.T)
    users, items = np.asarray(users0, dtype=np.float64), np.asarray(items0, dtype=np.float64)
    for _ in range(n_iterations):
        users = half_sweep64(x, items, alpha, reg)
        if trace is not None:
            trace.append(loss64(x, users, items, alpha, reg))
        items = half_sweep64(xt, users, alpha, reg)
        if trace is not None:
            trace.append(loss64(x, users, items, alpha, reg))
    return users, items


def loss64(x, users, items, alpha, reg):
    """sum_ui c_ui (p_ui - x_u . y_i)^2 + reg (||X||_F^2 + ||Y||_F^2), dense, float64"""
    x = canonical(x)
    users, items = np.asarray(users, dtype=np.float64), np.asarray(items, dtype=np.float64)
    d = np.asarray(x.todense(), dtype=np.float64)
    c = np.where(d != 0, float(alpha) * d, 1.0)
    p = (d != 0).astype(np.float64)
    return float((c * (p - users @ items.T) ** 2).sum() + float(reg) * ((users ** 2).sum() + (items ** 2).sum()))


def gram32(y, reg):
    """Y^T Y + reg I in float32, rows added one after the other"""
    y = np.asarray(y, dtype=np.float32)
    g = np.zeros((y.shape[1], y.shape[1]), dtype=np.float32)
    for k in range(y.shape[0]):
        g += np.outer(y[k], y[k])
    g[np.diag_indices_from(g)] += np.float32(reg)
    return g


def half_sweep32(x: sp.csr_matrix, y, alpha, g):
    """the yardstick: float32 throughout, the row's terms added one after the other in CSR order, then LAPACK's float32 Cholesky.
    ``g``: float32 [f, f]. (Step k adds the k-th entry of every row that has one, all those rows at once: the order within a row is the
    CSR order, and the rows are independent.)"""
    x = canonical(x)
    y = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))
    n, f = x.shape[0], y.shape[1]
    nnz = np.diff(x.indptr)
    order = np.argsort(-nnz, kind='stable')                                        # the rows with a k-th entry: a prefix of this order
    a = torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).repeat(n, 1, 1)
    b = torch.zeros(n, f, dtype=torch.float32)
    for k in range(int(nnz.max(initial=0))):
        cnt = int((nnz > k).sum())
        pos = x.indptr[order[:cnt]] + k
        ys = y[torch.from_numpy(x.indices[pos].astype(np.int64))]
        c = torch.from_numpy(np.float32(alpha) * x.data[pos].astype(np.float32))
        a[:cnt].addcmul_(((c - 1)[:, None] * ys)[:, :, None], ys[:, None, :])
        b[:cnt].addcmul_(c[:, None], ys)
    out = np.zeros((n, f), dtype=np.float32)
    for s in range(int((nnz > 0).sum())):
        sol = scipy.linalg.cho_solve(scipy.linalg.cho_factor(a[s].numpy(), lower=True, check_finite=False), b[s].numpy(), check_finite=False)
        assert sol.dtype == np.float32
        out[order[s]] = sol
    return out


def fit32(x, users0, items0, alpha, reg, n_iterations):
    x = canonical(x)
    xt = canonical(x.T)
    users, items = np.asarray(users0, dtype=np.float32), np.asarray(items0, dtype=np.float32)
    for _ in range(n_iterations):
        users = half_sweep32(x, items, alpha, gram32(items, reg))
        items = half_sweep32(xt, users, alpha, gram32(users, reg))
    return users, items


def backward_error(x: sp.csr_matrix, y, g, alpha, got):
    """max over the non-empty rows of ||A_r x_r - b_r||_inf / (||A_r||_inf ||x_r||_inf + ||b_r||_inf), all in float64 from the fp32 inputs"""
    x = canonical(x)
    got = np.asarray(got, dtype=np.float64)
    worst = 0.0
    for r in range(x.shape[0]):
        if x.indptr[r + 1] == x.indptr[r]:
            continue
        a, b = system64(x, r, y, g, alpha)
        res = np.abs(a @ got[r] - b).max()
        worst = max(worst, res / (np.abs(a).sum(axis=1).max() * np.abs(got[r]).max() + np.abs(b).max()))
        assert np.isfinite(res), f'row {r} is not finite'
    return worst


def world(n, m, density, seed, weighted=False) -> sp.csr_matrix:
    """a random n x m matrix with row 1 empty, row 2 holding a single entry and row 3 full (m entries: several staging chunks). The item
    half-sweep of a case runs on ``world(m, n, ...)``, the matrix in the place of X^T, so that it meets the same three rows."""
    rng = np.random.default_rng(seed)
    d = (rng.random((n, m)) < density).astype(np.float64)
    d[3] = 1
    if weighted:
        d *= rng.integers(1, 6, size=(n, m))
    d[1] = 0
    d[2] = 0
    d[2, m // 2] = 3 if weighted else 1
    x = canonical(sp.csr_matrix(d))
    nr = np.diff(x.indptr)
    assert nr[1] == 0 and nr[2] == 1 and nr[3] == m
    return x


def uniform_factors(n, f, seed):
    return np.random.RandomState(seed).uniform(-0.5 / f, 0.5 / f, size=(n, f)).astype(np.float32)
