"""EASE in numpy: the float64 restatement of ``fit`` (algorithms/linear_algs.py:148-160) and the blocked symmetric sweep of
csrc/ease.hip step for step. At ``dtype=np.float32`` the sweep is the yardstick for the kernel's rounding: its error against a float64
inverse is what an fp32 implementation of this method costs, whatever the summation order inside the three products. A plain module: no
fixtures, no pytest hooks."""
import json
import os

import numpy as np
import scipy.sparse as sp

LAMS = (1, 10, 500.7)                    # the g23 cases; int(500.7) = 500 reaches the diagonal
TOP_K = 10
FACTOR = 8                               # kernel error <= FACTOR * e_ref: another fixed summation order, fma chains in the update
MAX_LEFT_OUT = 0.10                      # of the users, for the near-tie rule of the top-k comparison


def gram(inter, lam):
    x = sp.csr_matrix(inter).astype(np.float64)
    g = np.asarray((x.T @ x).todense(), dtype=np.float64)
    g[np.diag_indices(g.shape[0])] += int(lam)
    return g


def weights(p):
    """linear_algs.py:157-158 in the dtype of ``p``: column j divided by -p[j, j], zero diagonal"""
    b = p / (-np.diag(p))
    b[np.diag_indices(b.shape[0])] = 0
    return b


def fit64(inter, lam):
    """-> (B, pred_mtx), float64"""
    b = weights(np.linalg.inv(gram(inter, lam)))
    return b, np.asarray(sp.csr_matrix(inter).astype(np.float64) @ b)


def gauss_jordan(d):
    """in-place unpivoted Gauss-Jordan inverse of a small SPD block, step p for every (i, j) at once, in the dtype of ``d``
    -> (inverse, index of the first pivot <= 0 or not finite, or -1)"""
    d = d.copy()
    bad = -1
    with np.errstate(all='ignore'):
        for p in range(d.shape[0]):
            piv = d[p, p]
            if bad < 0 and not (piv > 0 and np.isfinite(piv)):
                bad = p
            r = d.dtype.type(1) / piv
            rp = d[p, :] * r
            cp = d[:, p].copy()
            d -= np.outer(cp, rp)
            d[p, :] = rp
            d[:, p] = -cp * r
            d[p, p] = r
    return d, bad


def sweep_inverse(a, block=64, dtype=np.float64, return_info=False):
    """The inverse of a symmetric positive definite matrix by the blocked symmetric sweep. Per pivot block K:
    D^-1 = gauss_jordan(A[K, K]); P = A[K, :]; R = D^-1 P; A[J, J] -= P[:, J]^T R[:, J]; A[K, :] = R; A[:, K] = R^T; A[K, K] = -D^-1.
    After the last block A = -inverse. info: 1 + index of the first bad pivot, 0 if none."""
    a = np.array(a, dtype=dtype)
    n = a.shape[0]
    info = 0
    with np.errstate(all='ignore'):
        for k0 in range(0, n, block):
            k = slice(k0, min(k0 + block, n))
            dinv, bad = gauss_jordan(a[k, k])
            if bad >= 0 and info == 0:
                info = 1 + k0 + bad
            p = a[k, :].copy()
            r = dinv @ p
            a -= p.T @ r
            a[k, :] = r
            a[:, k] = r.T
            a[k, k] = -dinv
    a = -a
    return (a, info) if return_info else a


def e_ref(a):
    """max |sweep_inverse(a, float32) - inv64(a)|: the error of the method in fp32 on this matrix"""
    return float(np.abs(sweep_inverse(a, dtype=np.float32).astype(np.float64) - np.linalg.inv(np.asarray(a, dtype=np.float64))).max())


def e_ref_weights(g):
    """the same for the weights: max |weights(sweep_inverse(g, float32)) - weights(inv64(g))|, the epilogue in fp32 too"""
    b32 = weights(sweep_inverse(g, dtype=np.float32))
    assert b32.dtype == np.float32
    return float(np.abs(b32.astype(np.float64) - weights(np.linalg.inv(g))).max())


def masked_topk(pred, inter, k=TOP_K):
    """exact top-k of float64 score rows with the users' own interactions excluded -> (sorted scores desc [n, items], order [n, items])"""
    s = np.where(np.asarray(sp.csr_matrix(inter).todense()) != 0, -np.inf, pred)
    order = np.argsort(-s, axis=1, kind='stable')
    return np.take_along_axis(s, order, axis=1), order


def countable_users(pred, inter, err_b, k=TOP_K):
    """users whose float64 gap between the k-th and (k+1)-th score exceeds 2 * FACTOR * err_b * (their row count): an implementation
    whose weights are within FACTOR * err_b of the float64 ones cannot swap those two"""
    s, _ = masked_topk(pred, inter, k)
    counts = np.diff(sp.csr_matrix(inter).indptr)
    return (s[:, k - 1] - s[:, k]) > 2 * FACTOR * err_b * counts


def random_spd(n, lam, seed):
    """X^T X + lam I from a random 0/1 X [3 n, n] of density 0.15 -> float64"""
    rng = np.random.default_rng(seed)
    x = (rng.random((3 * n, n)) < 0.15).astype(np.float64)
    return x.T @ x + lam * np.eye(n)


def load_g23():
    """(arrays, cases) of tests/golden/g23_ease.{npz,json}"""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    with np.load(os.path.join(here, 'g23_ease.npz')) as f:
        arrays = {k: f[k] for k in f.files}
    return arrays, json.load(open(os.path.join(here, 'g23_ease.json')))['cases']
