"""References for NGCF's layer (csrc/ngcf.hip: ``sbr_ngcf_layer_fwd`` / ``sbr_ngcf_layer_bwd``, ``ops.ngcf_layer``, ``ops.NGCFLayerFn``,
``ops.NGCFPropagateFn``, ngcf.py) and the worlds its tests share. A plain module: numpy and torch on the CPU, no fixtures, no GPU. The
graph, the worlds, the clean propagation and ``fma32`` are tests/lightgcn_ref.py's, the uniforms tests/simgcl_ref.py's ``noise_ref``.

Definitions (float64). s = A^ x (lightgcn_ref), a = s + x, b = s * x, z = a W1 + b W2 + bias, h0 = z > 0 ? z : slope z,
h = keep ? h0 * inv_keep : 0 (keep[r][j] = U(seed, stream_id, r, j) >= p; inv_keep is the fp32 number 1 / (1 - p)), n = max(|h|_2, 1e-12),
out = h / n. The model's table is [E0 | out_1 | ... | out_L] with E_l = h_l; layer l (1-based) draws from stream_id = l.

The fp32 restatement ``layer32`` follows include/sibrar_hip.h one operation per line and is asked for bit for bit. ``layer_bwd32`` is
the backward entry's formulas in fp32 numpy; the order of its sums over rows is the kernel's only up to the tile (the fold adds
workgroup partials in double), so it is compared inside tolerances, never bit for bit.

Error bound of one layer against float64 on the same fp32 inputs and the same mask (u = 2^-24, gamma_k = k u / (1 - k u)), elementwise:
  s: bs of ``lightgcn_ref.propagate_bound``;
  a = fl(s^ + x): ba = bs + u (|s*| + bs + |x|);   b = fl(s^ x): bb = bs |x| + u (|s*| + bs) |x|;
  z: 2 Din fmaf and one addition, every term passes at most 2 Din + 1 roundings:
      bz = ba |W1| + bb |W2| + gamma_(2 Din + 1) ((|a*| + ba) |W1| + (|b*| + bb) |W2| + |bias|);
  h0: LeakyReLU with 0 < slope <= 1 is 1-Lipschitz (also where z^ and z* differ in sign) and slope z^ rounds once:
      bh0 = bz + u (|z*| + bz);   h = fl(h0^ inv_keep) where kept: bh = inv_keep (bh0 + u (|h0*| + bh0)), 0 where dropped (and bh0 at p = 0);
  q^ = the computed sum of squares: a product rounded once, then at most 4 ceil(Dout / 64) additions inside its partial sum and 4 of the
      butterfly, all terms non-negative: q^ = sum h^_j^2 (1 + t), |t| <= gamma_K, K = 4 ceil(Dout / 64) + 5; the root halves a
      relative error (bounded by the whole) and rounds once; | |h^| - |h*| | <= |bh|_2; the clamp is 1-Lipschitz:
      bn = |bh|_2 + gamma_(K + 1) (|h*|_2 + |bh|_2);
  out = fl(h^ / n^) with n^ >= lo = max(n* - bn, 1e-12):  bout = bh / lo + |h*| bn / (lo n*) + u (|h*| + bh) / lo.
Nothing here underflows: the tests' values are of the order 1e-3 .. 1e2."""
import functools

import numpy as np
import torch
import torch.nn.functional as Fn

import lightgcn_ref as L
import simgcl_ref as SG

F32 = np.float32
U = L.U
gamma = L.gamma
CLAMP = 1e-12
MAX_WIDTH = 128
USERS, ITEMS = (1, 63, 257), (1, 64, 130)
WIDTHS = ((1, 1), (3, 5), (4, 4), (63, 65), (64, 64), (65, 33), (64, 128), (128, 64), (128, 128))
RATES = (0.0, 0.3)
SLOPE = 0.2


def inv_keep32(p):
    return F32(1.0) / (F32(1.0) - F32(p))


def keep_mask(seed, stream, rows, d, p):
    """bool [len(rows), d]: u >= p with u keyed as sbr_graph_propagate_noise_f32 keys it; all True at p == 0 (no draw)"""
    if p == 0:
        return np.ones((len(rows), d), dtype=bool)
    return SG.noise_ref(seed, stream, rows, d) >= F32(p)


def sumsq32(h):
    """the header's order, fp32 at every step: float32 [rows, D] -> float32 [rows]"""
    h = np.ascontiguousarray(h, dtype=F32)
    rows, d = h.shape
    m = -(-d // 64)
    pad = np.zeros((rows, m * 64), dtype=F32)                                # columns past D contribute +0
    pad[:, :d] = h
    blocks = pad.reshape(rows, m, 16, 4)                                     # column j = 64 m + 4 l + c belongs to partial sum l
    t = np.zeros((rows, 16), dtype=F32)
    for k in range(m):
        for c in range(4):
            sq = blocks[:, k, :, c] * blocks[:, k, :, c]                     # h * h
            t = t + sq                                                       # t = t + (h * h)
    lanes = np.arange(16)
    for o in (1, 2, 4, 8):
        t = t + t[:, lanes ^ o]                                              # every t_l becomes t_l + t_(l xor o)
    assert t.dtype == F32 and bool((t == t[:, :1]).all())
    return t[:, 0]


def layer32(g, x, W1, W2, bias, slope=SLOPE, p=0.0, seed=0, stream=0, rows=None, s=None):
    """sbr_ngcf_layer_fwd restated -> {'s', 'z', 'h', 'out'} fp32 for the rows of ``rows=(r0, r1)`` (None: all); ``s``: the rows'
    propagated table when the caller has it already"""
    x, W1, W2, bias = (np.ascontiguousarray(t, dtype=F32) for t in (x, W1, W2, bias))
    r0, r1 = (0, g.n) if rows is None else rows
    if s is None:
        s = L.propagate32(g, x, rows=(r0, r1))[0][r0:r1]                     # s = y of sbr_graph_propagate_f32
    xr = x[r0:r1]
    a = s + xr                                                               # a = s + x
    b = s * xr                                                               # b = s * x
    acc = np.zeros((r1 - r0, W1.shape[1]), dtype=F32)                        # acc starts at +0.f
    for k in range(W1.shape[0]):
        acc = L.fma32(a[:, k:k + 1], W1[k][None, :], acc)                    # acc = fmaf(a[k], W1[k][j], acc)
    for k in range(W2.shape[0]):
        acc = L.fma32(b[:, k:k + 1], W2[k][None, :], acc)                    # acc = fmaf(b[k], W2[k][j], acc)
    z = acc + bias[None, :]                                                  # z = acc + bias[j]
    h = np.where(z > 0, z, F32(slope) * z).astype(F32)                       # z > 0 ? z : slope * z
    if p > 0:
        keep = keep_mask(seed, stream, np.arange(r0, r1), h.shape[1], p)
        h = np.where(keep, h * inv_keep32(p), F32(0.0)).astype(F32)          # kept: h * inv_keep; dropped: +0
    n = np.maximum(np.sqrt(sumsq32(h)), F32(CLAMP)).astype(F32)              # fmaxf(sqrtf(q), 1e-12f)
    out = h / n[:, None]                                                     # h / nrm
    assert z.dtype == F32 and h.dtype == F32 and out.dtype == F32
    return {'s': s, 'z': z, 'h': h, 'out': out}


def layer64(g, x, W1, W2, bias, slope=SLOPE, keep=None, inv_keep=1.0):
    """the definitions in float64 on the fp32 inputs; ``keep``: the mask (None: no dropout); slope and inv_keep as the fp32 numbers"""
    x, W1, W2, bias = (np.asarray(t, dtype=np.float64) for t in (x, W1, W2, bias))
    s = L.propagate64(g, x)
    a, b = s + x, s * x
    z = a @ W1 + b @ W2 + bias
    h0 = np.where(z > 0, z, float(F32(slope)) * z)
    h = h0 if keep is None else np.where(keep, h0 * float(inv_keep), 0.0)
    n = np.maximum(np.sqrt((h * h).sum(1)), CLAMP)
    return {'s': s, 'a': a, 'b': b, 'z': z, 'h0': h0, 'h': h, 'n': n, 'out': h / n[:, None]}


def layer_bound(g, x, W1, W2, bias, ref, keep=None, inv_keep=1.0):
    """-> {'z', 'h', 'out'}: the elementwise bounds of the module docstring; ``ref``: ``layer64`` of the same operands"""
    x, W1, W2, bias = (np.abs(np.asarray(t, dtype=np.float64)) for t in (x, W1, W2, bias))
    din, dout = W1.shape
    bs, _ = L.propagate_bound(g, x)
    s = np.abs(ref['s'])
    ba = bs + U * (s + bs + x)
    bb = bs * x + U * (s + bs) * x
    bz = ba @ W1 + bb @ W2 + gamma(2 * din + 1) * ((np.abs(ref['a']) + ba) @ W1 + (np.abs(ref['b']) + bb) @ W2 + bias)
    bh0 = bz + U * (np.abs(ref['z']) + bz)
    if keep is None:
        bh = bh0
    else:
        bh = np.where(keep, float(inv_keep) * (bh0 + U * (np.abs(ref['h0']) + bh0)), 0.0)
    k = 4 * -(-dout // 64) + 5
    l2 = np.sqrt((bh * bh).sum(1))
    bn = l2 + gamma(k + 1) * (np.sqrt((ref['h'] ** 2).sum(1)) + l2)
    lo = np.maximum(ref['n'] - bn, CLAMP)[:, None]
    habs = np.abs(ref['h'])
    bout = bh / lo + habs * bn[:, None] / (lo * ref['n'][:, None]) + U * (habs + bh) / lo
    return {'z': bz, 'h': bh, 'out': bout}


def layer_bwd32(g, x, W1, W2, slope, p, seed, stream, h, g_out, g_h=None):
    """sbr_ngcf_layer_bwd's formulas in fp32 numpy (sums in numpy's order: compared inside tolerances)
    -> {'ds', 'dx_direct', 'dx', 'dW1', 'dW2', 'dbias'}"""
    x, W1, W2, h, g_out = (np.ascontiguousarray(t, dtype=F32) for t in (x, W1, W2, h, g_out))
    s = L.propagate32(g, x)[0]
    q = sumsq32(h)
    root = np.sqrt(q)
    n = np.maximum(root, F32(CLAMP))[:, None]
    flag = (root >= F32(CLAMP)).astype(F32)[:, None]
    o = h / n
    dot = (g_out * o).sum(1, keepdims=True, dtype=F32) * flag
    dh = (g_out - o * dot) / n
    if g_h is not None:
        dh = dh + np.asarray(g_h, dtype=F32)
    if p > 0:
        dh = np.where(keep_mask(seed, stream, np.arange(g.n), h.shape[1], p), dh * inv_keep32(p), F32(0.0))
    dz = np.where(h > 0, dh, F32(slope) * dh).astype(F32)
    da, db = dz @ W1.T, dz @ W2.T
    ds, dxd = da + db * x, da + db * s
    return {'ds': ds, 'dx_direct': dxd, 'dx': dxd + L.propagate32(g, ds)[0], 'dW1': (s + x).T @ dz, 'dW2': (s * x).T @ dz, 'dbias': dz.sum(0)}


# ---- worlds and tables -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def world(n_users, n_items):
    return L.world(n_users, n_items)


def weights(din, dout, seed=0):
    """(W1, W2, bias): Xavier-sized weights, a bias of the order of the activations"""
    rng = np.random.default_rng(7000 + 131 * din + dout + seed)
    lim = np.sqrt(6.0 / (din + dout))
    return (rng.uniform(-lim, lim, (din, dout)).astype(F32), rng.uniform(-lim, lim, (din, dout)).astype(F32),
            (rng.standard_normal(dout) / 8).astype(F32))


SEED, STREAM = 0x1234_5678_9ABC, (3 << 32) + 5                             # both halves of both words are in use


@functools.lru_cache(maxsize=None)
def case(n_users, n_items, din, dout, p):
    """the operands of one forward case with both references and the bound, computed once and shared (read only)"""
    g = world(n_users, n_items)
    x = L.table(g.n, din, 11)
    W1, W2, bias = weights(din, dout)
    got = layer32(g, x, W1, W2, bias, SLOPE, p, SEED, STREAM, s=_s32(n_users, n_items, din))
    keep = None if p == 0 else keep_mask(SEED, STREAM, np.arange(g.n), dout, p)
    ref = layer64(g, x, W1, W2, bias, SLOPE, keep, inv_keep32(p))
    return {'g': g, 'x': x, 'W1': W1, 'W2': W2, 'bias': bias, 'r32': got, 'r64': ref, 'keep': keep,
            'bound': layer_bound(g, x, W1, W2, bias, ref, keep, inv_keep32(p))}


@functools.lru_cache(maxsize=None)
def _s32(n_users, n_items, din):
    g = world(n_users, n_items)
    return L.propagate32(g, L.table(g.n, din, 11))[0]


# ---- torch (float64: the truth; float32: the yardstick) ----------------------------------------------------------------------------------
def layer_torch(a_hat, x, W1, W2, bias, slope, keep, inv_keep):
    """one layer on the autograd tape in the dtype of ``x``; ``keep``: a bool tensor or None -> (h, out)"""
    s = a_hat @ x
    z = (s + x) @ W1 + (s * x) @ W2 + bias
    h = Fn.leaky_relu(z, float(F32(slope)))
    if keep is not None:
        h = torch.where(keep, h * float(inv_keep), torch.zeros_like(h))
    return h, Fn.normalize(h, dim=1, eps=CLAMP)


def layer_grads_torch(g, x, W1, W2, bias, slope, keep, inv_keep, g_out, g_h, dtype):
    """gradients of <out, g_out> + <h, g_h> (g_h None: the first term alone) -> {'dx', 'dW1', 'dW2', 'dbias'} in ``dtype``"""
    a = torch.from_numpy(g.a_hat()).to(dtype)
    ts = [torch.tensor(np.asarray(t), dtype=dtype, requires_grad=True) for t in (x, W1, W2, bias)]
    h, out = layer_torch(a, *ts, slope, None if keep is None else torch.from_numpy(keep), inv_keep)
    loss = (out * torch.tensor(np.asarray(g_out), dtype=dtype)).sum()
    if g_h is not None:
        loss = loss + (h * torch.tensor(np.asarray(g_h), dtype=dtype)).sum()
    loss.backward()
    return dict(zip(('dx', 'dW1', 'dW2', 'dbias'), (t.grad for t in ts)))


def param_names(n_layers):
    return ['user_embeddings.weight', 'item_embeddings.weight'] + [f'{k}.{l}' for l in range(n_layers) for k in ('w_gc', 'w_bi', 'b')]


def model_params(g, d, layer_sizes, seed=0):
    """a state_dict of numpy arrays for a model over ``g``: tables of the order 1/2 (as lightgcn_ref.model_world), Xavier weights"""
    rng = np.random.default_rng(90 + seed)
    sd = {'user_embeddings.weight': (rng.standard_normal((g.n_users, d)) / 2).astype(F32),
          'item_embeddings.weight': (rng.standard_normal((g.n_items, d)) / 2).astype(F32)}
    widths = (d,) + tuple(layer_sizes)
    for l, (a, b) in enumerate(zip(widths[:-1], widths[1:])):
        sd[f'w_gc.{l}'], sd[f'w_bi.{l}'], sd[f'b.{l}'] = weights(a, b, seed=l)
    return sd


def model_masks(g, layer_sizes, p, seed):
    """the masks a training forward of the model draws: layer l (1-based) from stream_id = l; None at p == 0"""
    if p == 0:
        return [None] * len(layer_sizes)
    return [keep_mask(seed, l + 1, np.arange(g.n), w, p) for l, w in enumerate(layer_sizes)]


def table_torch(a_hat, sd, n_layers, slope, masks, inv_keep):
    x = torch.cat([sd['user_embeddings.weight'], sd['item_embeddings.weight']], 0)
    parts = [x]
    for l in range(n_layers):
        keep = None if masks[l] is None else torch.from_numpy(masks[l])
        x, out = layer_torch(a_hat, x, sd[f'w_gc.{l}'], sd[f'w_bi.{l}'], sd[f'b.{l}'], slope, keep, inv_keep)
        parts.append(out)
    return torch.cat(parts, 1)


def model_torch(g, sd, u_idx, i_idx, labels, n_layers, slope, masks, inv_keep, dtype):
    """-> {'logits', 'loss', every parameter's gradient under its state_dict key} by torch autograd in ``dtype`` on the CPU"""
    a = torch.from_numpy(g.a_hat()).to(dtype)
    sd = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in sd.items()}
    e = table_torch(a, sd, n_layers, slope, masks, inv_keep)
    u = e[torch.from_numpy(u_idx)]
    i = e[g.n_users + torch.from_numpy(i_idx)]
    logits = (u[:, None, :] * i).sum(-1)
    loss = L.bpr(logits, torch.from_numpy(labels))
    loss.backward()
    return {'logits': logits.detach(), 'loss': loss.detach(), **{k: v.grad for k, v in sd.items()}}


def table64(g, sd, n_layers, slope=SLOPE):
    """the eval-mode representation table in float64, numpy"""
    with torch.no_grad():
        t = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in sd.items()}
        return table_torch(torch.from_numpy(g.a_hat()), t, n_layers, slope, [None] * n_layers, 1.0).numpy()


def table_bound(g, sd, n_layers, slope=SLOPE):
    """A bound of |table - table64| for the eval-mode table (float64 [n, W]): layer l's input already carries an error e, which the
    layer passes on through its Lipschitz constants and to which it adds ``layer_bound``'s own terms. With |dz| <= (A^ e + e) |W1| +
    (A^ e |x| + (|s| + A^ e) e) |W2| for an input error e (products of the errors included), LeakyReLU 1-Lipschitz, the normalisation
    as in the module docstring."""
    a = g.a_hat()
    x = np.concatenate([np.asarray(sd['user_embeddings.weight'], np.float64), np.asarray(sd['item_embeddings.weight'], np.float64)])
    e = np.zeros_like(x)
    parts = [e]
    for l in range(n_layers):
        W1, W2, bias = (np.asarray(sd[f'{k}.{l}'], np.float64) for k in ('w_gc', 'w_bi', 'b'))
        ref = layer64(g, x, W1, W2, bias, slope)
        own = layer_bound(g, np.abs(x) + e, W1, W2, bias, ref)               # the own terms at the computed input's magnitude
        ae = a @ e
        carried = (ae + e) @ np.abs(W1) + (ae * (np.abs(x) + e) + (np.abs(ref['s']) + ae) * e) @ np.abs(W2)
        bh = own['h'] + carried * (1 + U)
        k = 4 * -(-W1.shape[1] // 64) + 5
        l2 = np.sqrt((bh * bh).sum(1))
        bn = l2 + gamma(k + 1) * (np.sqrt((ref['h'] ** 2).sum(1)) + l2)
        lo = np.maximum(ref['n'] - bn, CLAMP)[:, None]
        habs = np.abs(ref['h'])
        parts.append(bh / lo + habs * bn[:, None] / (lo * ref['n'][:, None]) + U * (habs + bh) / lo)
        x, e = ref['h'], bh
    return np.concatenate(parts, 1)
