"""References for the noisy propagation of SimGCL / XSimGCL (csrc/graph_prop.hip: ``sbr_graph_propagate_noise_f32``,
``ops.graph_propagate_noise``, ``ops.NoisyPropagateFn``, simgcl.py). A plain module: numpy and torch on the CPU, no fixtures, no GPU. The
graph, the worlds and the clean propagation are tests/lightgcn_ref.py's, the generator is tests/naive_ref.py's.

Definitions (float64). With p = A^ x (lightgcn_ref), u[r][d] = U(seed, stream_id, r, d) in [0, 1) and n_r = max(|u_r|_2, 1e-12):
    y[r][d] = p + sign(p) * eps * u / n_r          (sign(0) = 0: torch.sign),
layer k of view v of step s draws from stream_id = s * 256 + v * 64 + k, E_k = perturb_k(A^ E_(k-1)), the table is the mean of the layers
1 .. L (layer 0 left out) and ``kept`` is E_keep_layer.

The fp32 restatement ``propagate_noise32`` follows include/sibrar_hip.h one operation per line: p by ``lightgcn_ref.propagate32``, the
squared norm in the header's order (``sumsq32``: G4 partial sums over blocks of four columns, then the xor butterfly from the widest offset
down), one square root, then eps * u, the division, the sign and the addition, each rounded to fp32 on its own.

Error bound of one noisy propagation against float64 on the same fp32 inputs (u = 2^-24, gamma_k = k u / (1 - k u)); eps is taken as
the fp32 number it is passed as, the uniforms are exact in both precisions:
  q^ = the computed sum of squares: every term is rounded once as a product and then passes at most 4 ceil(B / G4) additions inside
    its partial sum (B = ceil(D / 4) blocks) and log2(G4) additions of the butterfly; all terms are non-negative, so
    q^ = q (1 + a), |a| <= gamma_K with K = 4 ceil(B / G4) + log2(G4) + 1 (at most 15);
  n^ = fl(sqrt(q^)): the root halves a relative error (bounded here by the whole of it) and rounds once: n^ = n (1 + b),
    |b| <= gamma_(K + 1); the clamp at 1e-12 is monotone and does not raise a relative error;
  t^ = fl(fl(eps u) / n^) = t (1 + c), |c| <= gamma_(2 + 2 (K + 1)) (a quotient of error factors, Higham, Accuracy and Stability of
    Numerical Algorithms, lemma 3.3); the sign is exact;
  y^ = fl(p^ + sgn t^): |y^ - y*| <= bp + gamma_(2K + 4) t + u (|p*| + bp + (1 + gamma_(2K + 4)) t)
with bp the bound of ``lightgcn_ref.propagate_bound`` on p and t = eps u / n in float64 — as long as p^ and p* have the same sign. Where
|p*| <= bp the computed p may have the other sign, or be zero where p* is not (and the other way round): the noise then differs by at most
2 t, and ``propagate_noise_bound`` returns that allowance separately with the mask of the elements it applies to. The running sum adds
one addition and one multiplication as in lightgcn_ref:
  |sum' - (sum + y*) sum_scale| <= |sum_scale| (by + gamma_2 (|sum| + |y*| + by)).
"""
import numpy as np
import torch
import torch.nn.functional as Fn

import lightgcn_ref as L
import naive_ref as N

F32 = np.float32
U = L.U
gamma = L.gamma
CLAMP = 1e-12


def stream_id(step, view, layer):
    assert 0 <= layer < 64 and 0 <= view < 4
    return step * 256 + view * 64 + layer


def noise_ref(seed, stream, rows, d):
    """float32 [len(rows), d]: key = the halves of seed, counter = (row, column / 4, stream low, stream high), word column % 4"""
    seed, stream = int(seed), int(stream)
    rows = np.asarray(rows, dtype=np.int64)
    nb = (d + 3) // 4
    ctr = np.zeros((len(rows), nb, 4), dtype=np.uint32)
    ctr[:, :, 0] = rows.astype(np.uint32)[:, None]
    ctr[:, :, 1] = np.arange(nb, dtype=np.uint32)[None, :]
    ctr[:, :, 2] = stream & 0xFFFFFFFF
    ctr[:, :, 3] = stream >> 32
    words = N.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    return N.unit_float(words.reshape(len(rows), nb * 4)[:, :d])


def group_of(d):
    """(B, G4): the blocks of four columns of a row of d columns and the number of partial sums"""
    nb = (d + 3) // 4
    g4 = 1
    while g4 < 64 and g4 < nb:
        g4 *= 2
    return nb, g4


def sumsq32(u):
    """the header's order, fp32 at every step: float32 [rows, D] -> float32 [rows]"""
    u = np.ascontiguousarray(u, dtype=F32)
    rows, d = u.shape
    nb, g4 = group_of(d)
    per = -(-nb // g4)                                                       # blocks per partial sum
    pad = np.zeros((rows, per * g4 * 4), dtype=F32)                          # columns past D contribute +0
    pad[:, :d] = u
    blocks = pad.reshape(rows, per, g4, 4)                                   # block b = j * g4 + l belongs to partial sum l
    t = np.zeros((rows, g4), dtype=F32)
    for j in range(per):
        for c in range(4):
            sq = blocks[:, j, :, c] * blocks[:, j, :, c]                     # u * u
            t = t + sq                                                       # t = t + (u * u)
    o = g4 // 2
    lanes = np.arange(g4)
    while o > 0:
        t = t + t[:, lanes ^ o]                                              # every t_l becomes t_l + t_(l xor o)
        o //= 2
    assert t.dtype == F32 and bool((t == t[:, :1]).all())                    # an addition commutes: every lane holds the same bits
    return t[:, 0]


def perturb32(p, eps, seed, stream, r0=0):
    """the perturbation of rows r0 .. of the finished fp32 table p"""
    p = np.ascontiguousarray(p, dtype=F32)
    u = noise_ref(seed, stream, np.arange(r0, r0 + p.shape[0]), p.shape[1])
    n = np.maximum(np.sqrt(sumsq32(u)), F32(CLAMP)).astype(F32)
    t = F32(eps) * u                                                         # eps * u
    t = t / n[:, None]                                                       # (...) / n_r
    sg = np.sign(p).astype(F32)
    t = sg * t                                                               # the sign: exact
    assert t.dtype == F32
    return np.where(sg != 0, p + t, p).astype(F32)                           # p + (...); a zero stays as it is


def propagate_noise32(g, x, eps, seed, stream, sum=None, sum_scale=1.0, rows=None):
    """sbr_graph_propagate_noise_f32 restated: -> (y, sum') fp32; rows outside ``rows`` are zeros in y and untouched in sum'"""
    r0, r1 = (0, g.n) if rows is None else rows
    y, _ = L.propagate32(g, x, rows=rows)
    y[r0:r1] = perturb32(y[r0:r1], eps, seed, stream, r0)
    out_sum = None if sum is None else np.array(sum, dtype=F32, copy=True)
    if out_sum is not None:
        t = out_sum[r0:r1] + y[r0:r1]
        out_sum[r0:r1] = t * F32(sum_scale)
    return y, out_sum


def noise64(eps, seed, stream, n_rows, d):
    """float64 [n_rows, d]: eps u / n_r with eps the fp32 number"""
    u = noise_ref(seed, stream, np.arange(n_rows), d).astype(np.float64)
    n = np.maximum(np.sqrt((u * u).sum(1)), CLAMP)
    return float(F32(eps)) * u / n[:, None]


def propagate_noise64(g, x, eps, seed, stream):
    p = L.propagate64(g, x)
    return p + np.sign(p) * noise64(eps, seed, stream, g.n, p.shape[1])


def propagate_noise_bound(g, x, eps, seed, stream, sum=None, sum_scale=1.0):
    """-> (by, bsum or None, near, slack): |y - y*| <= by + near * slack elementwise, ``near`` the elements whose float64 p lies within
    its own bound of zero (the sign may differ there) and slack = 2 t (the module docstring)"""
    d = np.asarray(x).shape[1]
    nb, g4 = group_of(d)
    k = 4 * -(-nb // g4) + int(np.log2(g4)) + 1
    bp, _ = L.propagate_bound(g, x)
    p = L.propagate64(g, x)
    t = noise64(eps, seed, stream, g.n, d)
    tt = np.where(p != 0, t, 0.0)
    gt = gamma(2 * k + 4)
    by = bp + gt * tt + U * (np.abs(p) + bp + (1 + gt) * tt)
    near = np.abs(p) <= bp
    bs = None
    if sum is not None:
        ystar = p + np.sign(p) * t
        bs = abs(float(F32(sum_scale))) * (by + gamma(2) * (np.abs(np.asarray(sum, dtype=np.float64)) + np.abs(ystar) + by))
    return by, bs, near & (bp > 0), 2 * t


def layers64(g, e0, n_layers, eps, seed, step, view):
    """[E_1, ..., E_L] in float64"""
    x, out = np.asarray(e0, dtype=np.float64), []
    a = g.a_hat()
    for k in range(1, n_layers + 1):
        p = a @ x
        x = p + np.sign(p) * noise64(eps, seed, stream_id(step, view, k), g.n, p.shape[1])
        out.append(x)
    return out


def mean64(g, e0, n_layers, eps, seed, step, view, keep_layer=None):
    """-> (the mean of the layers 1 .. L, E_keep_layer or None) in float64"""
    ls = layers64(g, e0, n_layers, eps, seed, step, view)
    return sum(ls) / n_layers, None if keep_layer is None else ls[keep_layer - 1]


def mean32(g, e0, n_layers, eps, seed, step, view, keep_layer=None):
    """ops.NoisyPropagateFn restated: the sum starts at zero, sum_scale 1 on inner layers and fp32(1 / L) on the last"""
    x = np.ascontiguousarray(e0, dtype=F32)
    acc, kept = np.zeros_like(x), None
    for k in range(1, n_layers + 1):
        x, acc = propagate_noise32(g, x, eps, seed, stream_id(step, view, k), acc, 1.0 if k < n_layers else 1.0 / n_layers)
        if k == keep_layer:
            kept = x
    return acc, kept


def clean_mean_bound(g, e0, n_layers):
    """A bound of |E - E*| for the clean (eps = 0) mean of the layers 1 .. L computed as ``mean32`` does, against ``mean64``:
    ``lightgcn_ref.mean_bound``'s recursion without layer 0 in the sum. Layer k adds gamma_(n + 5) A^ |x_(k-1)| to the error A^ carries
    over; the running sum (L additions, the first onto zero, one multiplication, 1 / L rounded once) adds at most gamma_(L + 2) of its
    magnitude."""
    a = g.a_hat()
    n = g.deg.astype(np.float64)[:, None]
    mag = np.abs(np.asarray(e0, dtype=np.float64))
    e = np.zeros_like(mag)
    total_e, total_mag = np.zeros_like(mag), np.zeros_like(mag)
    for _ in range(n_layers):
        e = a @ e + gamma(n + 5) * (a @ (mag + e))
        mag = a @ mag
        total_e, total_mag = total_e + e, total_mag + mag
    return (total_e + gamma(n_layers + 2) * (total_mag + total_e)) / n_layers


def horner64(g, g_mean, g_kept, n_layers, keep_layer):
    """dE0 = A^(c_1 + A^(c_2 + ... A^ c_L)) with c_k = g_mean / L + [k == keep_layer] g_kept, float64"""
    a = g.a_hat()

    def c(k):
        return g_mean / n_layers + (g_kept if k == keep_layer else 0.0)

    t = c(n_layers)
    for k in range(n_layers, 1, -1):
        t = c(k - 1) + a @ t
    return a @ t


# ---- the two networks in torch (float64: the truth; float32: the yardstick) -------------------------------------------------------------
def layers_torch(a, e0, n_layers, eps, seed, step, view, dtype):
    """[E_1 .. E_L] on the autograd tape: the noise is a constant, the sign is torch.sign's (derivative zero)"""
    x, out = e0, []
    for k in range(1, n_layers + 1):
        p = a @ x
        noise = torch.from_numpy(noise64(eps, seed, stream_id(step, view, k), p.shape[0], p.shape[1])).to(dtype)
        x = p + torch.sign(p) * noise
        out.append(x)
    return out


def info_nce_half(a, b, tau):
    """half the symmetric InfoNCE (oracle/model_ref.py ``info_nce``) of the L2-normalised views, mean over the rows"""
    a, b = Fn.normalize(a, dim=-1), Fn.normalize(b, dim=-1)
    logits = a @ b.t() / tau
    target = torch.arange(logits.shape[0])
    return 0.5 * (Fn.cross_entropy(logits, target) + Fn.cross_entropy(logits.t(), target))


def model_torch(kind, g, uw, iw, u_idx, i_idx, labels, n_layers, dtype, eps=0.1, cl_weight=0.2, tau=0.2, seed=0, step=0, keep_layer=1):
    """``kind``: 'simgcl' or 'xsimgcl' -> {'logits', 'reg_loss', 'cl_u', 'cl_i', 'loss', 'user_embeddings.weight' (gradient),
    'item_embeddings.weight' (gradient), 'n_users', 'n_items' (distinct rows of the contrast)} by torch autograd in ``dtype`` on the CPU"""
    a = torch.from_numpy(g.a_hat()).to(dtype)
    uw = torch.tensor(np.asarray(uw), dtype=dtype, requires_grad=True)
    iw = torch.tensor(np.asarray(iw), dtype=dtype, requires_grad=True)
    e0 = torch.cat([uw, iw], 0)

    def mean(view, e):
        ls = layers_torch(a, e0, n_layers, e, seed, step, view, dtype)
        return sum(ls) / n_layers, ls

    if kind == 'xsimgcl':
        table, ls = mean(0, eps)
        va, vb = table, ls[keep_layer - 1]
    else:
        table, va, vb = mean(0, 0.0)[0], mean(1, eps)[0], mean(2, eps)[0]
    u = table[torch.from_numpy(u_idx)]
    i = table[g.n_users + torch.from_numpy(i_idx)]
    logits = (u[:, None, :] * i).sum(-1)
    users = torch.from_numpy(np.unique(u_idx))
    items = torch.from_numpy(np.unique(i_idx[:, 0])) + g.n_users
    cl_u, cl_i = info_nce_half(va[users], vb[users], tau), info_nce_half(va[items], vb[items], tau)
    reg = cl_weight * (cl_u + cl_i)
    loss = L.bpr(logits, torch.from_numpy(labels)) + reg
    loss.backward()
    return {'logits': logits.detach(), 'reg_loss': reg.detach(), 'cl_u': cl_u.detach(), 'cl_i': cl_i.detach(), 'loss': loss.detach(),
            'user_embeddings.weight': uw.grad, 'item_embeddings.weight': iw.grad, 'n_users': len(users), 'n_items': len(items)}
