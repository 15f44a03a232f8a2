"""SLIM in numpy: the Gram-form restatement of the reference's per-item elastic net (algorithms/linear_algs.py:39-112: sklearn's
``ElasticNet`` with ``positive=True``, ``fit_intercept=False``, on the matrix with the target column zeroed) as csrc/slim.hip solves it —
cyclic coordinate descent in ascending order, sklearn's first stopping test — with the dtype as a parameter. At ``np.float32`` the loop is the
yardstick for the kernel's rounding: its distance from the float64 run of the same sweeps is what fp32 costs this method. Also the
objective, the KKT residual and the near-tie rule of the top-k comparison. A plain module: no fixtures, no pytest hooks."""
import json
import os

import numpy as np
import scipy.sparse as sp

PARAMS = ((0.01, 0.5, 500), (0.001, 0.1, 500), (0.1, 0.9, 500))         # the g26 cases: (alpha, l1_ratio, max_iter)
TOL = 1e-4                               # the reference's (linear_algs.py:78)
TOP_K = 10
FACTOR = 8                               # kernel error <= FACTOR * e_ref, the margin of tests/ease_ref.py
MAX_LEFT_OUT = 0.10                      # of the users, for the near-tie rule of the top-k comparison
OBJ_TOL = 1e-4                           # sklearn stops at gap <= tol * y.y: objectives (times n) agree within 1e-4 * G_jj


def gram(inter):
    x = sp.csr_matrix(inter).astype(np.float64)
    return np.ascontiguousarray((x.T @ x).toarray(), dtype=np.float64)


def penalties(n_users, alpha, l1_ratio):
    """(l1, l2) of the Gram form, in double: sklearn's penalties times the number of samples"""
    return float(n_users) * float(alpha) * float(l1_ratio), float(n_users) * float(alpha) * (1. - float(l1_ratio))


def cd_column(g, j, l1, l2, max_iter, tol=TOL, dtype=np.float64, skip=True):
    """Column j -> (w, n_iter, steps): n_iter the sweeps run, negated when max_iter was reached without meeting the stopping test; steps
    the coordinate steps with a non-zero change. ``g`` must already have the dtype. ``skip=False`` is the plain loop over every k;
    ``skip=True`` jumps to the next coordinate whose step can be non-zero (w_k > 0, or r_k > l1), which gives the same bits."""
    m = g.shape[0]
    l1, l2, tol = dtype(l1), dtype(l2), dtype(tol)
    zero = dtype(0)
    r = g[:, j].copy()
    r[j] = 0
    w = np.zeros(m, dtype)
    diag = np.diagonal(g)
    steps = 0
    for sweep in range(1, max_iter + 1):
        d_w_max = w_max = zero
        k = 0
        while k < m:
            if skip:
                nxt = np.flatnonzero((w[k:] > 0) | (r[k:] > l1))
                nxt = nxt[nxt + k != j]
                if nxt.size == 0:
                    break
                k += int(nxt[0])
            if k != j and diag[k] > 0:
                new = max((r[k] + diag[k] * w[k]) - l1, zero) / (diag[k] + l2)
                d = new - w[k]
                if d != 0:
                    r -= d * g[k]
                    w[k] = new
                    steps += 1
                d_w_max, w_max = max(d_w_max, abs(d)), max(w_max, abs(new))
            k += 1
        assert r.dtype == dtype and w.dtype == dtype
        if w_max == 0 or d_w_max <= tol * w_max:
            return w, sweep, steps
    return w, -max_iter, steps


def cd(g, l1, l2, max_iter, tol=TOL, dtype=np.float64, cols=None, skip=True):
    """All columns (or ``cols``) -> (W [m, len(cols)] with W[k, j] the weight of item k for target j, n_iter, steps)"""
    g = np.ascontiguousarray(g, dtype=dtype)
    cols = range(g.shape[0]) if cols is None else cols
    out = [cd_column(g, j, l1, l2, max_iter, tol, dtype, skip) for j in cols]
    w = np.stack([o[0] for o in out], axis=1) if out else np.zeros((g.shape[0], 0), dtype)
    return w, np.array([o[1] for o in out], dtype=np.int64), np.array([o[2] for o in out], dtype=np.int64)


def e_ref(g, l1, l2, max_iter, cols=None):
    """(max |cd float32 - cd float64| at tol = 0, so that both run the same sweeps; the float64 weights; the float32 weights)"""
    w64 = cd(g, l1, l2, max_iter, 0., np.float64, cols)[0]
    w32 = cd(g, l1, l2, max_iter, 0., np.float32, cols)[0]
    assert w32.dtype == np.float32
    return (float(np.abs(w32.astype(np.float64) - w64).max()) if w64.size else 0.), w64, w32


def objective(g, j, w, l1, l2):
    """sklearn's objective of column j times n: 1/2 (G_jj - 2 w.q + w.G w) + l1 sum(w) + 1/2 l2 w.w, float64; w_j must be 0"""
    g = np.asarray(g, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    assert w[j] == 0
    q = g[:, j].copy()
    q[j] = 0
    return 0.5 * (g[j, j] - 2 * (w @ q) + w @ g @ w) + l1 * w.sum() + 0.5 * l2 * (w @ w)


def kkt_residual(g, j, w, l1, l2):
    """max over k != j with G_kk > 0 of |(G w - q)_k + l2 w_k + l1| where w_k > 0, and of its negative part where w_k = 0 (float64)"""
    g = np.asarray(g, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    q = g[:, j].copy()
    q[j] = 0
    grad = g @ w - q + l2 * w + l1
    live = (np.arange(len(w)) != j) & (np.diagonal(g) > 0)
    pos, zero = live & (w > 0), live & (w == 0)
    return max(float(np.abs(grad[pos]).max()) if pos.any() else 0., float(np.maximum(-grad[zero], 0).max()) if zero.any() else 0.)


def kkt_all(g, w, l1, l2, cols=None):
    cols = range(np.shape(g)[0]) if cols is None else cols
    return max((kkt_residual(g, j, np.asarray(w)[:, i], l1, l2) for i, j in enumerate(cols)), default=0.)


def masked_topk(pred, inter, k=TOP_K):
    """exact top-k of float64 score rows with the users' own interactions excluded -> (sorted scores desc [n, items], order [n, items])"""
    s = np.where(np.asarray(sp.csr_matrix(inter).todense()) != 0, -np.inf, pred)
    order = np.argsort(-s, axis=1, kind='stable')
    return np.take_along_axis(s, order, axis=1), order


def countable_users(pred_ref, pred_opt, inter, w_err, k=TOP_K):
    """The users for whom a model within ``w_err`` of the optimum's weights must give the reference's top-k. The reference's own weights
    stop up to a few 1e-4 from the optimum (random order, tol = 1e-4, and two of its runs differ as much), which a bound over all
    entries would turn into a gap that a third of the users miss. So the rule takes the two recorded score matrices as they are: a user
    counts when the top-k set of ``pred_ref`` (the reference's ``pred_mtx``) is the top-k set of ``pred_opt`` (``inter @ W_opt``) and the k-th
    place is safe in ``pred_opt``. It is safe when the float64 gap to the (k+1)-th score exceeds 2 * w_err * (the user's row count), so
    that weights within ``w_err`` of ``W_opt`` cannot swap those two. Under a heavy L1 penalty most weights are exactly zero and a user has
    fewer than k non-zero scores; then the place is also safe when the k-th score is an exact 0 in both matrices, both have their zeros
    at the same unseen items, and the smallest positive score exceeds the same bound: the positive items lead, and the exact zeros
    follow in ascending item index, the evaluation's rule for equal scores (a model that puts a non-zero weight where the optimum has
    none fails the comparison)."""
    s, order = masked_topk(pred_opt, inter, k)
    s_ref, order_ref = masked_topk(pred_ref, inter, k)
    same = np.array([set(a) == set(b) for a, b in zip(order[:, :k], order_ref[:, :k])])
    bound = 2 * w_err * np.diff(sp.csr_matrix(inter).indptr)
    unseen = np.asarray(sp.csr_matrix(inter).todense()) == 0
    zeros_agree = (((np.asarray(pred_opt) == 0) == (np.asarray(pred_ref) == 0)) | ~unseen).all(axis=1)
    least_positive = np.where(s > 0, s, np.inf).min(axis=1)
    zero_tail = (s[:, k - 1] == 0) & (s_ref[:, k - 1] == 0) & zeros_agree & (least_positive > bound)
    return same & (((s[:, k - 1] - s[:, k]) > bound) | zero_tail)


def world(n, m, density, seed, empty_item=None, twin=None):
    """a random 0/1 matrix [n, m] -> csr float64; ``empty_item``: an item nobody holds; ``twin=(a, b)``: item b holds what item a holds"""
    d = np.random.default_rng(seed).random((n, m)) < density
    if twin is not None:
        d[:, twin[1]] = d[:, twin[0]]
    if empty_item is not None:
        d[:, empty_item] = False
    x = sp.csr_matrix(d.astype(np.float64))
    x.sort_indices()
    return x


def case_name(alpha, l1_ratio):
    return f'a{alpha}_r{l1_ratio}'


def load_g26():
    """(arrays, cases) of tests/golden/g26_slim.{npz,json}"""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    with np.load(os.path.join(here, 'g26_slim.npz')) as f:
        arrays = {k: f[k] for k in f.files}
    return arrays, json.load(open(os.path.join(here, 'g26_slim.json')))['cases']
