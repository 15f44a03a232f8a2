"""References for DirectAU's loss terms (csrc/directau.hip, ``ops.uniformity``, ``ops.UniformityFn``, ``ops.AlignLossFn``, directau.py): the
definitions in float64, the kernel's formula restated in numpy float32, and the error bounds the tests hold the kernel to. No test
functions; a plain module (no test module imports another, so the little of LightGCN's propagation that the model needs is restated).

Definitions (x [n, D], t > 0):  d_ij^2 = |x_i - x_j|^2,  w_ij = exp(-t d_ij^2),  S = sum_{i<j} w_ij,  loss = log(S * 2 / (n (n - 1))),
    dloss/dx_i = (-2 t / S) (x_i sum_{j != i} w_ij - sum_{j != i} w_ij x_j).

The bound, derived from the kernel as built (u = 2^-24, factor 1.01 for second order):
  d^2 in Gram form, (sq_i + sq_j) - 2 g_ij: sq is 32 fmaf chains of at most ceil(D / 32) terms and a 5-level butterfly, g one fmaf chain
      of D terms, then one addition and one subtraction (2 g is exact): |delta d^2| <= (D + 3) u (|x_i| + |x_j|)^2. The clamp at 0 only
      moves the value towards the truth (d^2 >= 0).
  the exponent -(t d^2) is rounded once more, u t d^2 <= u t (|x_i| + |x_j|)^2, and expf is allowed EXP_ULP = 4 u (2 ulp; the HIP
      device library documents 1): a term's relative error is at most  r = t (D + 4) u max_ij (|x_i| + |x_j|)^2 + 4 u.
  the sum of positive terms: a thread adds its 16 terms of a tile pair in a tree of depth 4 in fp32; everything after that (over the
      column tiles, the lanes, the waves, the row tiles) is added in double, whose roundings (at most tiles + 8 + tiles of 2^-53 each)
      are below one u in total, and S is rounded to fp32 once: chain depth 4 + 1 + 1 = 6:  rS = 1.01 (r + 6 u).
  loss = log(S * 2 / (n (n - 1))) is computed in double from the fp32 S and rounded once: |delta loss| <= rS + 2 u |loss|.
  the gradient: coef = g * (-2 t / S) (three fp32 roundings on top of rS); rs_i adds per column tile 2 tree levels, 4 butterfly levels
      and one running addition: depth tiles + 6; acc_i[d] is one fmaf chain over j of n terms. With
      M_i[d] = |x_i[d]| rs_i + sum_j w_ij |x_j[d]|:   |delta dx_i[d]| <= 1.01 |coef| M_i[d] (r + rS + (n + tiles + 12) u).
  The bound is usable (it is the conditioning of the difference x_i rs_i - acc_i, not a figure read off the kernel), so the tests use
  it for the gradient too; FACTOR times the error of the float32 restatement against float64 is what the model's table gradients are
  held to, where the bound would have to pass through the lookups' scatter as well."""
import numpy as np
import torch

F32 = np.float32
U = 2.0 ** -24
EXP_ULP = 4 * U
SECOND = 1.01
FACTOR = 8.0
TILE = 64


def tiles(n):
    return (n + TILE - 1) // TILE


# ---- float64 -----------------------------------------------------------------------------------------------------------------------------
def _w64(x, t):
    x = np.asarray(x, dtype=np.float64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    w = np.exp(-t * d2)
    np.fill_diagonal(w, 0.0)
    return x, w


def uniformity64(x, t):
    """-> (loss, S) in float64"""
    x, w = _w64(x, t)
    n = x.shape[0]
    S = np.triu(w, 1).sum()
    return float(np.log(S * 2.0 / (n * (n - 1)))), float(S)


def uniformity_grad64(x, t, g=1.0):
    x, w = _w64(x, t)
    S = np.triu(w, 1).sum()
    return g * (-2.0 * t / S) * (x * w.sum(1)[:, None] - w @ x)


def align64(logits, labels, scale):
    logits, labels = np.asarray(logits, dtype=np.float64), np.asarray(labels, dtype=np.float64)
    return float(scale * ((2.0 - 2.0 * logits) * (labels == 1)).sum())


# ---- the kernel's formula in numpy float32 -----------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c) of fp32 operands, exactly: the product is exact in float64, the sum is rounded to odd before the fp32 rounding"""
    p = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    p, c = np.broadcast_arrays(p, c)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    odd = np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return odd.astype(F32)


def _sq32(x):
    n, D = x.shape
    ss = np.zeros((n, 32), dtype=F32)
    for d0 in range(0, D, 32):
        v = np.zeros((n, 32), dtype=F32)
        v[:, :min(32, D - d0)] = x[:, d0:d0 + 32]
        ss = fma32(v, v, ss)
    lane = np.arange(32)
    for o in (16, 8, 4, 2, 1):
        ss = (ss + ss[:, lane ^ o]).astype(F32)
    return ss[:, 0]


def _w32(x, t):
    """the pair weights as the kernel forms them, fp32 [n, n], zero on the diagonal"""
    x = np.ascontiguousarray(x, dtype=F32)
    n, D = x.shape
    sq = _sq32(x)
    g = np.zeros((n, n), dtype=F32)
    for d in range(D):
        g = fma32(x[:, d][:, None], x[:, d][None, :], g)
    d2 = np.maximum(F32(0), (sq[:, None] + sq[None, :]).astype(F32) - F32(2) * g).astype(F32)
    w = np.exp(-(F32(t) * d2).astype(F32)).astype(F32)
    np.fill_diagonal(w, F32(0))
    return x, w


def _row4(w):
    """((w0 + w1) + (w2 + w3)) over groups of four columns: [.., 4 k] -> [.., k]"""
    q = w.reshape(w.shape[:-1] + (-1, 4))
    return ((q[..., 0] + q[..., 1]).astype(F32) + (q[..., 2] + q[..., 3]).astype(F32)).astype(F32)


def _pad(w):
    n = w.shape[0]
    p = np.zeros((tiles(n) * TILE,) * 2, dtype=F32)
    p[:n, :n] = w
    return p


def uniformity32(x, t):
    """-> (loss, S) fp32, in the kernel's order up to the double-precision sums (added here by numpy in float64)"""
    x, w = _w32(x, t)
    n = x.shape[0]
    p = _pad(np.triu(w, 1))
    c4 = _row4(p)                                                              # [rows, 16 T]: a thread's four columns of a row
    r = c4.reshape(-1, 4, c4.shape[1])
    thread = ((r[:, 0] + r[:, 1]).astype(F32) + (r[:, 2] + r[:, 3]).astype(F32)).astype(F32)   # a thread's 16 terms of every tile pair
    S = F32(thread.astype(np.float64).sum())
    return F32(np.log(np.float64(S) * 2.0 / (float(n) * float(n - 1)))), S


def uniformity_grad32(x, t, S, g=1.0):
    x, w = _w32(x, t)
    n, D = x.shape
    T = tiles(n)
    c4 = _row4(_pad(w))[:n].reshape(n, T, 16)                                  # per column tile, the row's 16 threads
    lane = np.arange(16)
    rs = np.zeros(n, dtype=F32)
    for ct in range(T):
        v = c4[:, ct]
        for o in (1, 2, 4, 8):
            v = (v + v[:, lane ^ o]).astype(F32)
        rs = (rs + v[:, 0]).astype(F32)
    acc = np.zeros((n, D), dtype=F32)
    for j in range(n):
        acc = fma32(w[:, j][:, None], x[j][None, :], acc)
    coef = F32(g) * (F32(-2) * F32(t) / F32(S)).astype(F32)
    return (F32(coef) * ((x * rs[:, None]).astype(F32) - acc).astype(F32)).astype(F32)


# ---- the bounds --------------------------------------------------------------------------------------------------------------------------
def term_rel(x, t):
    x = np.asarray(x, dtype=np.float64)
    D = x.shape[1]
    nrm = np.sqrt((x * x).sum(1))
    two = np.sort(nrm)[-2:].sum()                                              # max over pairs of |x_i| + |x_j|
    return t * (D + 4) * U * two * two + EXP_ULP


def s_rel(x, t):
    return SECOND * (term_rel(x, t) + 6 * U)


def loss_bound(x, t):
    loss, _ = uniformity64(x, t)
    return s_rel(x, t) + 2 * U * abs(loss)


def grad_bound(x, t, g=1.0):
    """float64 [n, D]"""
    xx, w = _w64(x, t)
    n = xx.shape[0]
    S = np.triu(w, 1).sum()
    m = np.abs(xx) * w.sum(1)[:, None] + w @ np.abs(xx)
    return SECOND * abs(g) * (2.0 * t / S) * m * (term_rel(x, t) + s_rel(x, t) + (n + tiles(n) + 12) * U)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def rows(n, D, seed, unit=True, max_norm=2.0, dup=0.0):
    """n rows of width D: unit rows, or rows of norms spread over (0.25, max_norm]; ``dup``: that share of the rows are copies of others"""
    rng = np.random.default_rng(1000 * n + D + seed)
    x = rng.standard_normal((n, D))
    x /= np.sqrt((x * x).sum(1, keepdims=True))
    if not unit:
        x *= rng.uniform(0.25, max_norm, size=(n, 1))
        x[0] *= max_norm / np.sqrt((x[0] * x[0]).sum())
    k = int(round(dup * n))
    if k:
        dst = rng.choice(n, size=k, replace=False)
        src = rng.choice(np.setdiff1d(np.arange(n), dst), size=k)                  # the originals stay as they are: n - k distinct rows
        x[dst] = x[src]
    x = x.astype(F32)
    if unit:                                                                   # as the model passes them: normalised in fp32
        x = (x / np.sqrt((x.astype(np.float64) ** 2).sum(1, keepdims=True))).astype(F32)
    return x


# ---- the model's step in torch (float64: the truth; float32: the yardstick for the table gradients) ----------------------------------------
def a_hat(m):
    """dense float64 D^-1/2 A D^-1/2 of the bipartite graph of the users x items 0/1 matrix ``m`` over the joint rows (users first):
    tests/lightgcn_ref.py's definition, restated"""
    m = np.asarray(m, dtype=np.float64)
    nu, ni = m.shape
    a = np.zeros((nu + ni, nu + ni))
    a[:nu, nu:] = m
    a[nu:, :nu] = m.T
    deg = a.sum(1)
    with np.errstate(divide='ignore'):
        s = np.where(deg > 0, 1.0 / np.sqrt(deg), 0.0)
    return s[:, None] * a * s[None, :]


def mean_bound(m, e0, n_layers):
    """tests/lightgcn_ref.py's bound of |E - E*| for the L-layer mean, restated (float64 [n, D]): a layer adds gamma_(deg + 5) A^ |x| to
    the error A^ carries over, every running sum gamma_2 of its magnitude, 1 / (L + 1) one more u"""
    def gam(k):
        return k * U / (1 - k * U)
    a = a_hat(m)
    mm = np.asarray(m, dtype=np.float64)
    deg = np.concatenate([mm.sum(1), mm.sum(0)])[:, None]
    mag = np.abs(np.asarray(e0, dtype=np.float64))
    e = np.zeros_like(mag)
    total_e, total_mag = np.zeros_like(mag), mag.copy()
    for _ in range(n_layers):
        e = a @ e + gam(deg + 5) * (a @ (mag + e))
        mag = a @ mag
        total_e, total_mag = total_e + e, total_mag + mag
    return (total_e + gam(2 * n_layers + 1) * (total_mag + total_e)) / (n_layers + 1)


def uniformity_torch(x, t):
    n = x.shape[0]
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    iu = torch.triu_indices(n, n, 1)
    return torch.exp(-t * d2[iu[0], iu[1]]).mean().log()


def model_world(d, seed=0):
    """50 users x 40 items, a batch of 37 with repeated users and repeated positive items, 3 negatives
    -> (matrix, user table, item table, u_idx, i_idx, labels)"""
    rng = np.random.default_rng(70 + seed)
    m = (rng.random((50, 40)) < 0.2).astype(np.float64)
    m[7] = 0
    m[:, 11] = 0
    uw = (rng.standard_normal((50, d)) / 2).astype(F32)
    iw = (rng.standard_normal((40, d)) / 2).astype(F32)
    u = rng.integers(0, 50, size=37)
    u[3] = u[9] = u[20] = 5
    i = rng.integers(0, 40, size=(37, 4))
    i[4, 0] = i[8, 0] = i[30, 0] = 13
    labels = np.zeros((37, 4), dtype=np.float64)
    labels[:, 0] = 1
    return m, uw, iw, u.astype(np.int64), i.astype(np.int64), labels


def step_torch(m, uw, iw, u_idx, i_idx, labels, n_layers, gamma, t, dtype):
    """One training step's terms and table gradients by torch autograd in ``dtype`` on the CPU, the definitions only
    -> {'align', 'uniform_u', 'uniform_i', 'reg', 'logits', 'user_embeddings.weight', 'item_embeddings.weight', 'u_hat', 'i_hat'}"""
    nu = uw.shape[0]
    uw = torch.tensor(np.asarray(uw), dtype=dtype, requires_grad=True)
    iw = torch.tensor(np.asarray(iw), dtype=dtype, requires_grad=True)
    x = torch.cat([uw, iw], 0)
    acc = x
    if n_layers:
        a = torch.from_numpy(a_hat(m)).to(dtype)
        for _ in range(n_layers):
            x = a @ x
            acc = acc + x
    e = acc / (n_layers + 1)
    u = e[torch.from_numpy(u_idx)]
    i = e[nu + torch.from_numpy(i_idx)]
    uh = u / u.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    ih = i / i.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    logits = (uh[:, None, :] * ih).sum(-1)
    lab = torch.from_numpy(np.asarray(labels, dtype=np.float64))
    align = ((2 - 2 * logits.double()) * (lab == 1)).sum() / (lab == 1).sum()
    lu, li = uniformity_torch(uh, t), uniformity_torch(ih[:, 0], t)
    reg = gamma * (lu + li) / 2
    (align + reg.double()).backward()
    return {'align': align.detach(), 'uniform_u': lu.detach(), 'uniform_i': li.detach(), 'reg': reg.detach(), 'logits': logits.detach(),
            'user_embeddings.weight': uw.grad, 'item_embeddings.weight': iw.grad, 'u_hat': uh.detach(), 'i_hat': ih.detach()}


def hat_error(D, rel_in=0.0):
    """A bound of |x^ - x^*| (Euclidean, per row) for a row normalised in fp32 from an input that carries a relative error ``rel_in``
    (Euclidean): the sum of squares (D terms), the square root and the division add (D + 3) u / 2 + 2 u <= (D + 4) u, and the
    normalisation's Jacobian (I - x^ x^T) / |x| has norm 1 / |x|, so the input's error passes through unamplified"""
    return SECOND * ((D + 4) * U + rel_in)


def model_loss_bound(x_hat64, t, D, rel_in=0.0):
    """The uniformity bound pushed through the normalisation: the kernel's own bound on the rows it is given, plus what their error
    delta = hat_error moves the loss by: |delta d^2| <= 2 d (2 delta) + (2 delta)^2 with d <= 2, and |delta loss| <= t max |delta d^2|"""
    delta = hat_error(D, rel_in)
    return loss_bound(x_hat64, t) + SECOND * t * (8 * delta + 4 * delta * delta)


def yardstick(ref64, got32):
    """max |float32 on the CPU - float64| of one quantity, as measured: no floor"""
    return float((got32.double() - ref64).abs().max())
