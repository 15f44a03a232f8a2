"""P3alpha in numpy: the float64 restatement of ``fit`` (algorithms/graph_algs.py:26-72) as the three-factor product
``(D_u^-1 X)(D_i^-1 X^T)(D_u^-1 X)``, and the fp32 *order oracle* of csrc/p3alpha.hip: numpy float32 arithmetic in exactly the sequences
include/sibrar_hip.h states, so the kernels are compared with it bit for bit. The error bound of the fp32 model against float64 and the
near-tie rule of the top-k comparison follow from that order; neither is measured. A plain module: no fixtures, no pytest hooks."""
import json
import os

import numpy as np
import scipy.sparse as sp

ALPHAS = (1.9, 1.0, 0.5)                 # the g24 cases
TOP_K = 10
MAX_LEFT_OUT = 0.10                      # of the users, for the near-tie rule of the top-k comparison
U32 = 2.0 ** -24                         # unit roundoff of fp32
POW_ULP = 16                             # accuracy the OpenCL specification grants pow, in ulp; the device library follows it
F32 = np.float32


def _csr(inter):
    x = sp.csr_matrix(inter)
    x.sort_indices()
    return x


# ---- float64 -----------------------------------------------------------------------------------------------------------------------
def fit64(inter, alpha):
    """-> (W, pred_mtx), float64: W = D_i^-1 X^T D_u^-1 X and ((D_u^-1 X) W) ** alpha; empty users and items give zeros"""
    x = np.asarray(_csr(inter).todense(), dtype=np.float64)
    du, di = x.sum(axis=1), x.sum(axis=0)
    with np.errstate(divide='ignore'):
        iu, ii = np.where(du > 0, 1. / du, 0.), np.where(di > 0, 1. / di, 0.)
    w = (ii[:, None] * x.T) @ (iu[:, None] * x)
    return w, ((iu[:, None] * x) @ w) ** alpha


# ---- the order oracle -------------------------------------------------------------------------------------------------------------------
def inv32(d):
    """inv(d) = 1.0f / (float)d, correctly rounded (numpy's float32 division is)"""
    with np.errstate(divide='ignore'):
        return F32(1) / np.asarray(d).astype(F32)


def walk32(inter):
    """W as sbr_p3_walk_dense computes it: column j's accumulator starts at +0 and receives inv(d_v) over the users v of item i that hold
    j, ascending, by fp32 additions; stored as acc * inv(d_i), zeros for an item nobody holds -> float32 [m, m]"""
    x = _csr(inter)
    xt = _csr(x.T)
    n, m = x.shape
    inv_u, inv_i = inv32(np.diff(x.indptr)), inv32(np.diff(xt.indptr))
    w = np.zeros((m, m), dtype=F32)
    for i in range(m):
        users = xt.indices[xt.indptr[i]:xt.indptr[i + 1]]
        if len(users) == 0:
            continue
        acc = np.zeros(m, dtype=F32)
        for v in users:                                                        # ascending: sort_indices
            cols = x.indices[x.indptr[v]:x.indptr[v + 1]]                      # distinct: one addition per column and user
            acc[cols] = acc[cols] + inv_u[v]
        w[i] = acc * inv_i[i]
    assert w.dtype == F32
    return w


def pre_power32(inter, w32, rows=None):
    """score rows before the power, as sbr_p3_score_rows computes them: column j's accumulator starts at +0, receives W[i, j] over the
    user's items i ascending, then one multiplication by inv(d_u); a user without items gives zeros -> float32 [len(rows), m]"""
    x = _csr(inter)
    n, m = x.shape
    rows = np.arange(n) if rows is None else np.asarray(rows)
    inv_u = inv32(np.diff(x.indptr))
    out = np.zeros((len(rows), m), dtype=F32)
    for b, u in enumerate(rows):
        items = x.indices[x.indptr[u]:x.indptr[u + 1]]
        if len(items) == 0:
            continue
        acc = np.zeros(m, dtype=F32)
        for i in items:
            acc = acc + w32[i]
        out[b] = acc * inv_u[u]
    assert out.dtype == F32
    return out


def power64(pre32, alpha):
    """float64 pow of the (bit-known) fp32 pre-power values: what powf is compared with, to POW_ULP ulp"""
    return np.asarray(pre32, dtype=np.float64) ** alpha


def ulp32(x):
    """spacing of fp32 at |x| (float64 array, normal range)"""
    x = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(x)) - 23)


# ---- the bound ------------------------------------------------------------------------------------------------------------------------
def rel_bound(inter, alpha):
    """Relative error bound of a fp32 score against the float64 one, per user [n, 1]:

        (1.01 * alpha * (max_i d_i + d_u + 3) * 2^-24 + 16 * 2^-23)

    Every term of both sums is positive, so sequential fp32 summation of k terms has relative error <= (k - 1) u (1 + O(k u)); the terms
    themselves carry one rounding each. W[i, j]: inv(d_v) (1 rounding), at most d_i additions (d_i - 1 roundings that count), times
    inv(d_i) (2 roundings: the division and the product): <= (d_i + 2) u. The score: at most d_u additions of such terms (d_u - 1), times
    inv(d_u) (2): in all <= (max_i d_i + d_u + 3) u to first order; the factor 1.01 covers the higher-order terms for every shape of the
    suite ((1 + u)^k - 1 <= 1.01 k u while k u < 0.01). The power multiplies a relative error by alpha (to first order, inside the same
    1.01), and powf itself adds 16 ulp = 16 * 2^-23 relative at most."""
    x = _csr(inter)
    d_u = np.diff(x.indptr).astype(np.float64)
    d_i_max = float(np.diff(_csr(x.T).indptr).max()) if x.shape[1] else 0.
    return (1.01 * alpha * (d_i_max + d_u + 3) * U32 + POW_ULP * 2.0 ** -23)[:, None]


def masked_topk(pred, inter, k=TOP_K):
    """exact top-k of float64 score rows with the users' own interactions excluded -> (sorted scores desc [n, items], order [n, items])"""
    s = np.where(np.asarray(_csr(inter).todense()) != 0, -np.inf, pred)
    order = np.argsort(-s, axis=1, kind='stable')
    return np.take_along_axis(s, order, axis=1), order


def countable_users(pred, inter, alpha, k=TOP_K):
    """users whose float64 scores at the k-th and (k+1)-th place lie further apart than the two allowed errors together:
    s_k (1 - b) > s_{k+1} (1 + b) with b the user's relative bound. An implementation within the bound cannot swap those two; a user
    whose k-th score is zero (tied with every other zero) does not count"""
    s, _ = masked_topk(pred, inter, k)
    b = rel_bound(inter, alpha)[:, 0]
    hi, lo = s[:, k - 1], np.maximum(s[:, k], 0.)                                # (-inf: fewer than k + 1 candidates)
    return (hi > 0) & (hi * (1 - b) > lo * (1 + b))


# ---- worlds of the GPU tests ---------------------------------------------------------------------------------------------------------
def world(name, base=None):
    """0/1 matrices with an empty user, an empty item, one user holding every (other) item and one item held by every (other) user.
    '50x40': ``base`` (the fixture's matrix) with those four planted; '300x200', '97x130': random, density 0.1"""
    if name == '50x40':
        d = np.asarray(base, dtype=bool).copy()
    else:
        n, m = (300, 200) if name == '300x200' else (97, 130)
        d = np.random.default_rng(n + m).random((n, m)) < 0.1
    n, m = d.shape
    d[3] = True                          # a user holding every item
    d[:, 5] = True                       # an item held by every user
    d[n - 2] = False                     # an empty user
    d[:, m - 3] = False                  # an empty item
    return _csr(d.astype(np.float64))


def load_g24():
    """(arrays, cases) of tests/golden/g24_p3alpha.{npz,json}"""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    with np.load(os.path.join(here, 'g24_p3alpha.npz')) as f:
        arrays = {k: f[k] for k in f.files}
    return arrays, json.load(open(os.path.join(here, 'g24_p3alpha.json')))['cases']
