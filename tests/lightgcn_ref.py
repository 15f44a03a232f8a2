"""References for LightGCN's propagation (csrc/graph_prop.hip, ``ops.graph_propagate``, ``ops.LightGCNPropagateFn``, lightgcn.py) and the
worlds its tests share. A plain module: numpy and torch on the CPU, no fixtures, no GPU.

Definitions (float64). X [U, I] is the 0/1 interaction matrix, A = [[0, X], [X^T, 0]] the adjacency of the joint row space (users first),
deg its row sums, s = deg^-1/2 (0 where deg = 0), A^ = diag(s) A diag(s). One propagation is y = A^ x; the model's table is
E = (1 / (L + 1)) sum_{k=0..L} A^^k E0; logits[b, n] = <E[u_b], E[U + i_bn]>; the loss is BPR (oracle/losses_ref.py:31-37 restated).

The fp32 restatement ``propagate32`` follows include/sibrar_hip.h one operation per line. fmaf is emulated in float64 as
tests/block_ref.py's ``fma32`` does (the product of two fp32 numbers is exact in float64), with one addition: the float64 sum is
rounded to odd before it is rounded to fp32 (the error of the sum is recovered by TwoSum; where it is not zero and the sum's last bit is
even, the sum moves one float64 step towards the error). A 53-bit round-to-odd result rounds to the same 24 bits as the exact value, so
the emulation has no double rounding and the GPU tests ask for bit equality on every input.

Error bound of one propagation against float64 on the same fp32 inputs, u = 2^-24, gamma_k = k u / (1 - k u), for row r of degree n and
m_r[d] = sum_c |s_r s_c x[c][d]| (the exact scales):
  s^_c = fl(1 / fl(sqrt(deg_c))): two roundings, s^_c = s_c (1 + t), |t| <= gamma_2; the same for s^_r;
  the chain of n fmaf: one rounding each, the first term sees all n of them: |acc - sum_c s^_c x_c| <= gamma_n sum_c |s^_c x_c|;
  y = fl(s^_r acc): one more rounding. Together every term carries at most 2 + n + 2 + 1 factors (1 + d), |d| <= u:
      |y - y*| <= gamma_(n + 5) m_r.
  sum' = fl(fl(sum + y) sum_scale), with sum and the fp32 sum_scale taken as given: one rounding each on top of y's error and |y*| <= m_r:
      |sum' - (sum + y*) sum_scale| <= |sum_scale| (gamma_(n + 7) m_r + gamma_2 |sum|).
Nothing here underflows: the tests' values are of the order 1e-2 .. 1e2."""
import numpy as np
import scipy.sparse as sp
import torch

F32 = np.float32
U = 2.0 ** -24


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1 - k * U)


def fma32(a, b, c):
    """fmaf(a, b, c) of fp32 operands, exactly (see the module docstring)"""
    p = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)          # exact: 24 + 24 bits
    c = np.asarray(c, dtype=np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                                                   # TwoSum: p + c = s + e exactly
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    odd = np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return odd.astype(F32)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


# ---- the graph ------------------------------------------------------------------------------------------------------------------------
class Graph:
    """``m``: users x items, 0/1 -> the two CSR forms the entry takes, the joint degrees and the joint neighbour lists"""

    def __init__(self, m):
        m = sp.csr_matrix(m).astype(np.float64)
        m.sum_duplicates()
        m.sort_indices()
        assert m.nnz == 0 or bool((m.data == 1).all())
        t = sp.csr_matrix(m.T)
        t.sort_indices()
        self.m, self.t = m, t
        self.n_users, self.n_items = m.shape
        self.n = self.n_users + self.n_items
        self.deg = np.concatenate([np.diff(m.indptr), np.diff(t.indptr)]).astype(np.int64)

    def neighbours(self, r):
        """joint rows of the neighbours of joint row r, in ascending CSR order"""
        if r < self.n_users:
            return self.n_users + self.m.indices[self.m.indptr[r]:self.m.indptr[r + 1]].astype(np.int64)
        i = r - self.n_users
        return self.t.indices[self.t.indptr[i]:self.t.indptr[i + 1]].astype(np.int64)

    def adjacency(self):
        return sp.bmat([[None, self.m], [self.t, None]], format='csr') if self.n_users and self.n_items else sp.csr_matrix((self.n, self.n))

    def s64(self):
        with np.errstate(divide='ignore'):
            return np.where(self.deg > 0, 1.0 / np.sqrt(self.deg.astype(np.float64)), 0.0)

    def a_hat(self):
        """dense float64 A^ [n, n]"""
        s = self.s64()
        return s[:, None] * np.asarray(self.adjacency().todense(), dtype=np.float64) * s[None, :]

    def s32(self):
        """the header's scale: a correctly rounded fp32 square root, then a correctly rounded fp32 division; +0 for an empty row"""
        root = np.sqrt(self.deg.astype(F32))
        with np.errstate(divide='ignore'):
            return np.where(self.deg > 0, F32(1.0) / root, F32(0.0)).astype(F32)


def propagate64(g: Graph, x):
    return g.a_hat() @ np.asarray(x, dtype=np.float64)


def mean64(g: Graph, e0, n_layers):
    a, x = g.a_hat(), np.asarray(e0, dtype=np.float64)
    acc = x.copy()
    for _ in range(n_layers):
        x = a @ x
        acc = acc + x
    return acc / (n_layers + 1)


def propagate32(g: Graph, x, sum=None, sum_scale=1.0, rows=None):
    """sbr_graph_propagate_f32 restated: -> (y, sum') fp32; rows outside ``rows=(r0, r1)`` come back as zeros in y and untouched in sum'"""
    x = np.ascontiguousarray(x, dtype=F32)
    s = g.s32()
    r0, r1 = (0, g.n) if rows is None else rows
    y = np.zeros_like(x)
    out_sum = None if sum is None else np.array(sum, dtype=F32, copy=True)
    scale = F32(sum_scale)
    nb = [g.neighbours(r) for r in range(r0, r1)]
    acc = np.zeros((r1 - r0, x.shape[1]), dtype=F32)                         # acc starts at +0.f
    for j in range(max([len(c) for c in nb], default=0)):                    # the j-th neighbour of every row that has one
        live = np.array([k for k, c in enumerate(nb) if len(c) > j], dtype=np.int64)
        c = np.array([nb[k][j] for k in live], dtype=np.int64)
        acc[live] = fma32(s[c][:, None], x[c], acc[live])                    # acc = fmaf(s_c, x[c][d], acc)
    y[r0:r1] = s[r0:r1, None] * acc                                          # y = s_r * acc
    if out_sum is not None:
        t = out_sum[r0:r1] + y[r0:r1]                                        # sum + y
        out_sum[r0:r1] = t * scale                                           # (...) * sum_scale
    return y, out_sum


def mean32(g: Graph, e0, n_layers):
    """ops.LightGCNPropagateFn restated: the sum seeded with e0, sum_scale 1 on inner layers and fp32(1 / (L + 1)) on the last"""
    x = np.ascontiguousarray(e0, dtype=F32)
    acc = x.copy()
    for k in range(1, n_layers + 1):
        x, acc = propagate32(g, x, acc, 1.0 if k < n_layers else 1.0 / (n_layers + 1))
    return acc


def propagate_bound(g: Graph, x, sum=None, sum_scale=1.0):
    """-> (bound of |y - y*|, bound of |sum' - (sum + y*) sum_scale| or None), float64 [n, D] (the module docstring)"""
    s = g.s64()
    absx = np.abs(np.asarray(x, dtype=np.float64))
    m = s[:, None] * (np.asarray(g.adjacency().todense(), dtype=np.float64) @ (s[:, None] * absx))
    n = g.deg.astype(np.float64)[:, None]
    by = gamma(n + 5) * m
    if sum is None:
        return by, None
    return by, abs(float(F32(sum_scale))) * (gamma(n + 7) * m + gamma(2) * np.abs(np.asarray(sum, dtype=np.float64)))


def mean_bound(g: Graph, e0, n_layers):
    """A bound of |E - E*| for the L-layer mean computed as ``mean32`` does, against ``mean64`` (float64 [n, D]): layer k's input
    already carries an error e_(k-1), which A^ (non-negative) carries over, and adds its own gamma_(n + 5) A^ |x_(k-1)| with the computed
    |x_(k-1)| <= |x*_(k-1)| + e_(k-1); every running sum adds gamma_2 of its magnitude (one addition, one multiplication; 1 / (L + 1)
    itself is rounded once: one more u), all of it bounded by sum_k A^^k |E0|."""
    a = g.a_hat()
    n = g.deg.astype(np.float64)[:, None]
    mag = np.abs(np.asarray(e0, dtype=np.float64))
    e = np.zeros_like(mag)
    total_e, total_mag = np.zeros_like(mag), mag.copy()
    for _ in range(n_layers):
        e = a @ e + gamma(n + 5) * (a @ (mag + e))
        mag = a @ mag
        total_e, total_mag = total_e + e, total_mag + mag
    return (total_e + gamma(2 * n_layers + 1) * (total_mag + total_e)) / (n_layers + 1)


# ---- worlds ---------------------------------------------------------------------------------------------------------------------------
USERS, ITEMS = (1, 5, 257), (3, 64, 130)
WIDTHS = (1, 3, 4, 63, 64, 65, 128, 256, 512)


def world(n_users, n_items, seed=0):
    """A random 0/1 matrix with, where the shape has room: an empty user row (the last user) and an empty item column (item 2),
    item 0 held by every other user (a long row on the item side), users 2 and 3 with exactly 64 and 65 items, items 4 and 5 with
    exactly 64 and 65 users."""
    rng = np.random.default_rng(1000 * n_users + n_items + seed)
    x = (rng.random((n_users, n_items)) < 0.12).astype(np.int8)
    x[:, 0] = 1
    if n_items >= 65 + 6 and n_users > 4:
        for u, k in ((2, 64), (3, 65)):
            x[u] = 0
            x[u, rng.choice(np.arange(6, n_items), size=k - 1, replace=False)] = 1
            x[u, 0] = 1
    if n_users >= 65 + 5 and n_items > 5:
        for i, k in ((4, 64), (5, 65)):
            x[:, i] = 0
            x[rng.choice(np.arange(4, n_users - 1), size=k, replace=False), i] = 1
    if n_items > 2:
        x[:, 2] = 0
    if n_users > 1:
        x[n_users - 1] = 0
    g = Graph(sp.csr_matrix(x))
    if n_items >= 71 and n_users > 4:
        assert g.deg[2] == 64 and g.deg[3] == 65
    if n_users >= 70 and n_items > 5:
        assert g.deg[n_users + 4] == 64 and g.deg[n_users + 5] == 65
    return g


def table(n, d, seed):
    return (np.random.default_rng(seed).standard_normal((n, d)) / 4).astype(F32)


def exact_world(seed=0, with_empty=False):
    """Complete bipartite blocks K_(a, b) with a, b in {1, 4, 16} (a block's users have degree b, its items degree a), the users and the
    items each shuffled: every degree is 1, 4 or 16 (``with_empty``: plus two users and one item without interactions), so every scale
    is 1, 1/2 or 1/4. With small-integer tables every product, every partial sum (at most 16 terms), the layer sum and the scaling by
    1 / (L + 1) for L in {1, 3} are exact in fp32: float64 and fp32 agree bit for bit whatever the order."""
    rng = np.random.default_rng(seed)
    blocks = [(a, b) for a in (1, 4, 16) for b in (1, 4, 16)] + [(1, 1), (4, 4), (16, 1)]
    n_u, n_i = sum(a for a, _ in blocks), sum(b for _, b in blocks)
    x = np.zeros((n_u + (2 if with_empty else 0), n_i + (1 if with_empty else 0)), dtype=np.int8)
    u0 = i0 = 0
    for a, b in blocks:
        x[u0:u0 + a, i0:i0 + b] = 1
        u0, i0 = u0 + a, i0 + b
    x = x[rng.permutation(x.shape[0])][:, rng.permutation(x.shape[1])]
    g = Graph(sp.csr_matrix(x))
    assert set(np.unique(g.deg)) <= ({0, 1, 4, 16} if with_empty else {1, 4, 16})
    return g


def int_table(n, d, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=(n, d)).astype(F32)


# ---- the model in torch (float64: the truth; float32: the yardstick of the model tests) -----------------------------------------------
def model_world(d, seed=0):
    """40 users x 30 items, a batch of 24 users with one positive and 4 negatives each -> (graph, user table, item table, u_idx, i_idx, labels)"""
    rng = np.random.default_rng(50 + seed)
    x = (rng.random((40, 30)) < 0.2).astype(np.int8)
    x[7] = 0
    x[:, 11] = 0
    g = Graph(sp.csr_matrix(x))
    uw = (rng.standard_normal((40, d)) / 2).astype(F32)
    iw = (rng.standard_normal((30, d)) / 2).astype(F32)
    u = rng.integers(0, 40, size=24)
    u[3] = u[9] = 5                                                            # users repeat within a batch
    i = rng.integers(0, 30, size=(24, 5))
    labels = np.zeros((24, 5), dtype=F32)
    labels[:, 0] = 1
    return g, uw, iw, u.astype(np.int64), i.astype(np.int64), labels


def bpr(logits, labels):
    """oracle/losses_ref.py:31-37 in the dtype of ``logits``"""
    diff = (logits[:, :1] - logits[:, 1:]).flatten()
    target = torch.repeat_interleave(labels[:, 0].to(logits.dtype), logits.shape[1] - 1)
    return (torch.clamp(diff, min=0) - diff * target + torch.log1p(torch.exp(-diff.abs()))).mean()


def model_torch(g: Graph, uw, iw, u_idx, i_idx, labels, n_layers, dtype):
    """-> {'logits', 'loss', 'user_embeddings.weight' (gradient), 'item_embeddings.weight' (gradient)} by torch autograd in ``dtype`` on
    the CPU: the definitions of the module docstring, nothing else"""
    a = torch.from_numpy(g.a_hat()).to(dtype)
    uw = torch.tensor(np.asarray(uw), dtype=dtype, requires_grad=True)
    iw = torch.tensor(np.asarray(iw), dtype=dtype, requires_grad=True)
    x = torch.cat([uw, iw], 0)
    acc = x
    for _ in range(n_layers):
        x = a @ x
        acc = acc + x
    e = acc / (n_layers + 1)
    u = e[torch.from_numpy(u_idx)]
    i = e[g.n_users + torch.from_numpy(i_idx)]
    logits = (u[:, None, :] * i).sum(-1)
    loss = bpr(logits, torch.from_numpy(labels))
    loss.backward()
    return {'logits': logits.detach(), 'loss': loss.detach(), 'user_embeddings.weight': uw.grad, 'item_embeddings.weight': iw.grad}


FACTOR = 8.0                              # the model tests allow FACTOR times the float32-on-the-CPU error (the SLIM tests' margin)


def yardstick(ref64, got32):
    """max |float32 on the CPU - float64| of one quantity, as measured: no floor. (The scalar loss needs none either: the engine's loss
    kernel adds its terms in float64, so its error is what the fp32 logits and the fp32 differences pos - neg carry into the mean, not
    the rounding of an fp32 scalar.)"""
    return float((got32.double() - ref64).abs().max())
