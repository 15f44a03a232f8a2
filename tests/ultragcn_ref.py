"""References for UltraGCN (csrc/ultragcn.hip, ``ops.cooc_weight_topk``, ``ops.ultragcn_scales``, ``ops.UltraGCNLossFn``, ultragcn.py). A plain
module: no fixtures, no pytest hooks, no GPU. The definitions are the authors' code as remembered.

(a) Float64 definitions. X 0/1 [n_users, n_items], degrees d_u, d_i, G = X^T X (diagonal included), g_i = sum_j G_ij = sum over the users of
item i of d_u. beta_u = sqrt(d_u + 1) / d_u (0 where d_u = 0), beta_i = 1 / sqrt(d_i + 1), row_scale = sqrt(g + 1) / g (0 where g = 0),
col_scale = 1 / sqrt(g + 1), omega_ij = G_ij row_scale_i col_scale_j. The list of item i: the K largest omega_ij with G_ij > 0 by (value
descending, index ascending), i itself included by default; (-1, 0) behind the length. With s(i) = <U[u], V[i]> and sp = softplus:
    L_pos = (w1 + w2 beta_u beta_p) sp(-s(p)),  L_neg = (1 / N) sum_c (w3 + w4 beta_u beta_jc) sp(s(j_c)),
    L_nbr = sum_{k < len[p]} omega[p, k] sp(-s(nbr[p, k])),  L = sum_b (L_pos + negative_weight L_neg + lam L_nbr).
coef = dL/ds per slot [B, 1 + N + K]: -(w1 + ..) sigmoid(-s), (negative_weight / N)(w3 + ..) sigmoid(s), -lam omega sigmoid(-s), 0 in padded slots.

(b) The float32 restatement of the list values: (float32(G_ij) * row_scale32[i]) * col_scale32[j], two numpy float32 multiplications (numpy
never fuses), and the same selection. The kernel's lists equal it bit for bit. Each value is within 2 u relative of the float64 product of
the same float32 scales (two roundings, gamma_2).

(c) The bound of the fused loss — derived from the kernel's operation order (include/sibrar_hip.h), never fitted. u = 2^-24, SECOND = 1.01
for second-order terms. Per slot, with A = sum_d |Ub_d V_d|:
    ds    <= gamma(D) A                       a dot product of D terms, however the chain and the butterfly split it
    expf, log1pf: 2 ulp = 4 u relative each (the allowance of tests/hip_testutil.py); +, *, / correctly rounded, u each
    sp    : |sp'| <= 1; e off by 4 u moves log1p(e) by <= 4 u e <= 8 u log1p(e) (log1p(e) >= e / 2 on [0, 1]), log1pf's own 4 u, one
            addition:  d sp <= ds + 13 u sp
    sig   : |sig'| = sig (1 - sig) <= min(1/4, sig); e's 4 u reaches 1 / (1 + e) halved and e / (1 + e) whole, then one addition and one
            division:  d sig <= min(1/4, sig) ds + 6 u sig
    w     : fl(w1), fl(w2) and three operations on positive terms in w1 + w2 * (bu * bi): 4 u at the most; cw up to 3 more (fl(negative_weight),
            the division by N, the product); coef = cw * sig one more: 4 + 3 + 6 + 1 = 14, taken as 16:
            d coef <= cw min(1/4, sig) ds + 16 u |coef|
    term  = w * sp, 4 + 13 + 1 = 18, taken as 20:  d term <= w ds + 20 u term; the sums run in double (nothing to add); each part and the
            total are rounded to float32 once (+ u |part|), and the total takes fl(negative_weight) and fl(lam) (+ u on those two products)
    dUb[d]  = chain of 1 + N + K terms: sum_c d coef_c |V_cd| + gamma(1 + N + K) sum_c |coef_c V_cd|
    dV[j,d] = chain over the n_j slots that name j, then one multiplication by grad (1 in the tests):
              sum d coef |Ub_d| + gamma(n_j + 1) sum |coef Ub_d|
The inputs (tables, beta, omega) are float32 numbers taken as exact: the float64 reference is evaluated on the same float32 inputs.

(d) fmaf in numpy: the product of two float32 numbers is exact in float64; the sum with the accumulator is rounded to odd in float64 (TwoSum
gives the error term) and then to nearest float32, which is the correctly rounded fused result (53 >= 2 * 24 + 2)."""
import numpy as np
import scipy.sparse as sp
import torch

U = 2.0 ** -24
SECOND = 1.01
FACTOR = 8.0                              # the model test allows FACTOR times the float32-on-the-CPU error (the SLIM tests' margin)


def gamma(t):
    t = np.asarray(t, dtype=np.float64)
    return t * U / (1 - t * U)


# ---- (a), (b): degrees, scales, lists -----------------------------------------------------------------------------------------------------
def dense01(x):
    x = x.toarray() if sp.issparse(x) else np.asarray(x)
    return (x != 0).astype(np.int64)


def degrees(x):
    """(d_u, d_i, g) as int64 from the sparse structure alone: g needs no Gram matrix"""
    x = sp.csr_matrix(x)
    d_u = np.diff(x.indptr).astype(np.int64)
    xt = sp.csr_matrix(x.T)
    d_i = np.diff(xt.indptr).astype(np.int64)
    g = np.array([d_u[xt.indices[xt.indptr[i]:xt.indptr[i + 1]]].sum() for i in range(xt.shape[0])], dtype=np.int64)
    return d_u, d_i, g


def scales64(x):
    """(beta_u, beta_i, row_scale, col_scale) float64"""
    d_u, d_i, g = (v.astype(np.float64) for v in degrees(x))
    with np.errstate(divide='ignore', invalid='ignore'):
        beta_u = np.where(d_u > 0, np.sqrt(d_u + 1) / d_u, 0.)
        row = np.where(g > 0, np.sqrt(g + 1) / g, 0.)
    return beta_u, 1 / np.sqrt(d_i + 1), row, 1 / np.sqrt(g + 1)


def scales32(x):
    return tuple(v.astype(np.float32) for v in scales64(x))


def omega64(x, row_scale=None, col_scale=None):
    """(omega float64 [m, m], G int64 [m, m]); the scales default to the float64 ones"""
    d = dense01(x)
    G = d.T @ d
    if row_scale is None:
        _, _, row_scale, col_scale = scales64(x)
    return G * np.asarray(row_scale, dtype=np.float64)[:, None] * np.asarray(col_scale, dtype=np.float64)[None, :], G


def values32(x, row_scale32, col_scale32):
    """(b): float32 [m, m], 0 where G_ij = 0"""
    d = dense01(x)
    G = d.T @ d
    assert row_scale32.dtype == np.float32 and col_scale32.dtype == np.float32 and G.max(initial=0) < 1 << 24
    v = G.astype(np.float32) * row_scale32[:, None]
    v = v * col_scale32[None, :]
    assert v.dtype == np.float32
    return v, G


def select(v, G, k, include_self=True, rows=None):
    """the canonical lists of a value matrix (any float dtype) -> (idx int32 [m, k], val [m, k] in v's dtype, len int32 [m]); rows outside
    ``rows=(r0, r1)`` stay empty"""
    m = v.shape[0]
    idx, val, length = np.full((m, k), -1, dtype=np.int32), np.zeros((m, k), dtype=v.dtype), np.zeros(m, dtype=np.int32)
    r0, r1 = (0, m) if rows is None else rows
    for i in range(r0, r1):
        ok = (G[i] > 0) & (v[i] > 0)
        if not include_self:
            ok[i] = False
        cand = np.flatnonzero(ok)
        order = cand[np.lexsort((cand, -v[i, cand].astype(np.float64)))][:k]
        length[i] = len(order)
        idx[i, :len(order)], val[i, :len(order)] = order, v[i, order]
    return idx, val, length


def lists32(x, row_scale32, col_scale32, k, include_self=True, rows=None):
    v, G = values32(x, row_scale32, col_scale32)
    return select(v, G, k, include_self, rows)


def brute_force_lists(v, G, k, include_self=True):
    """the same lists by a dense sort of whole rows: every column of the row sorted by (candidate first, value descending, index ascending)"""
    m = v.shape[0]
    out = []
    for i in range(m):
        triples = [(-float(v[i, j]), j) for j in range(m) if G[i, j] > 0 and v[i, j] > 0 and (include_self or j != i)]
        out.append([j for _, j in sorted(triples)][:k])
    return out


def has_value_tie(v, G):
    """a row holds two candidates of exactly equal value"""
    for i in range(v.shape[0]):
        c = v[i][(G[i] > 0) & (v[i] > 0)]
        if len(np.unique(c)) < len(c):
            return True
    return False


# ---- the fused loss in float64 --------------------------------------------------------------------------------------------------------------
def slot_items(i_idx, nbr_idx, nbr_len):
    """(items int64 [B, 1 + N + K] with -1 in padded slots, kind int [1 + N + K]: 0 positive, 1 negative, 2 neighbour)"""
    i_idx = np.asarray(i_idx, dtype=np.int64)
    B, n1 = i_idx.shape
    K = nbr_idx.shape[1]
    p = i_idx[:, 0]
    nb = np.asarray(nbr_idx, dtype=np.int64)[p].copy()
    nb[np.arange(K)[None, :] >= np.asarray(nbr_len)[p][:, None]] = -1
    return np.concatenate([i_idx, nb], axis=1), np.array([0] + [1] * (n1 - 1) + [2] * K)


def loss_torch(Ub, V, u_idx, i_idx, beta_u, beta_i, nbr_idx, nbr_val, nbr_len, sc, dtype=torch.float64):
    """The torch composition (gather, bmm, weighted softplus) in ``dtype``. Ub [B, D] and V [n_items, D] are torch leaves or plain arrays;
    sc = (w1, w2, w3, w4, negative_weight, lam). -> dict(parts [3], loss, scores [B, C], weights of the loss terms [B, C], mask [B, C])"""
    w1, w2, w3, w4, negw, lam = sc
    items, kind = slot_items(i_idx, nbr_idx, nbr_len)
    B, C = items.shape
    N = int((kind == 1).sum())
    mask = torch.from_numpy(items >= 0)
    safe = torch.from_numpy(np.where(items >= 0, items, 0))
    t = lambda a: a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a)).to(dtype)
    Ub, V = t(Ub).to(dtype), t(V).to(dtype)
    bu = t(np.asarray(beta_u, dtype=np.float64)[np.asarray(u_idx)]).to(dtype)[:, None]
    bi = t(np.asarray(beta_i, dtype=np.float64))[safe].to(dtype)
    p = np.asarray(i_idx)[:, 0]
    om = torch.zeros(B, C, dtype=dtype)
    om[:, 1 + N:] = t(np.asarray(nbr_val, dtype=np.float64)[p]).to(dtype)
    kd = torch.from_numpy(kind)[None, :]
    w = torch.where(kd == 0, w1 + w2 * bu * bi, torch.where(kd == 1, w3 + w4 * bu * bi, om)) * mask
    s = torch.bmm(V[safe], Ub[:, :, None])[:, :, 0]
    sgn = torch.where(kd == 1, 1., -1.).to(dtype)
    terms = w * torch.nn.functional.softplus(sgn * s) * mask
    pos, neg, nbr = terms[:, 0].sum(), terms[:, 1:1 + N].sum() / N, terms[:, 1 + N:].sum()
    return {'parts': torch.stack([pos, neg, nbr]), 'loss': pos + negw * neg + lam * nbr, 'scores': s, 'w': w, 'mask': mask, 'items': items,
            'kind': kind, 'sgn': sgn}


def analytic(r, sc):
    """coef [B, C] = dL/ds from the scores and weights of ``loss_torch`` (float64, no autograd)"""
    w1, w2, w3, w4, negw, lam = sc
    N = int((r['kind'] == 1).sum())
    kd = torch.from_numpy(r['kind'])[None, :]
    cw = torch.where(kd == 0, r['w'], torch.where(kd == 1, negw / N * r['w'], lam * r['w']))
    s = r['scores'].detach()
    return (r['sgn'] * cw * torch.sigmoid(r['sgn'] * s) * r['mask']).detach(), cw.detach()


def reference(Ub32, V32, u_idx, i_idx, beta_u32, beta_i32, nbr_idx, nbr_val32, nbr_len, sc):
    """Everything the kernel tests compare against, in float64 on the float32 inputs, with the bounds of (c): dict of
    (value, bound) pairs for 'parts', 'loss', 'coef', 'dUb', 'dV', plus 'scores'."""
    Ub = torch.from_numpy(np.asarray(Ub32, dtype=np.float64)).requires_grad_(True)
    V = torch.from_numpy(np.asarray(V32, dtype=np.float64)).requires_grad_(True)
    r = loss_torch(Ub, V, u_idx, i_idx, beta_u32, beta_i32, nbr_idx, nbr_val32, nbr_len, sc)
    r['loss'].backward()
    coef, cw = analytic(r, sc)
    w1, w2, w3, w4, negw, lam = sc
    items, kind, mask = r['items'], r['kind'], r['mask'].numpy()
    B, C = items.shape
    D = Ub.shape[1]
    N = int((kind == 1).sum())
    Un, Vn = np.abs(Ub.detach().numpy()), np.abs(V.detach().numpy())
    safe = np.where(items >= 0, items, 0)
    A = np.einsum('bd,bcd->bc', Un, Vn[safe]) * mask
    ds = SECOND * gamma(D) * A
    s = r['scores'].detach().numpy()
    sgn = r['sgn'].numpy()
    x = sgn * s
    spv = np.logaddexp(0., x) * mask
    sig = 1 / (1 + np.exp(-x))
    w = r['w'].detach().numpy()
    cwn, cf = cw.numpy() * mask, np.abs(coef.numpy())
    d_coef = SECOND * (cwn * np.minimum(0.25, sig) * ds + 16 * U * cf)
    d_term = SECOND * (w * ds + 20 * U * w * spv)
    parts = r['parts'].detach().numpy()
    b_parts = np.array([d_term[:, 0].sum(), d_term[:, 1:1 + N].sum() / N, d_term[:, 1 + N:].sum()]) + U * np.abs(parts)
    b_loss = b_parts[0] - U * abs(parts[0]) + negw * (b_parts[1] - U * abs(parts[1])) + lam * (b_parts[2] - U * abs(parts[2])) \
        + U * abs(float(r['loss'].detach())) + U * (negw * abs(parts[1]) + lam * abs(parts[2]))
    Vs = Vn[safe] * mask[:, :, None]
    b_dub = np.einsum('bc,bcd->bd', d_coef, Vs) + SECOND * gamma(C) * np.einsum('bc,bcd->bd', cf, Vs)
    n_items = V.shape[0]
    n_j = np.bincount(items[items >= 0], minlength=n_items).astype(np.float64)
    b_dv, mag = np.zeros((n_items, D)), np.zeros((n_items, D))
    flat = items.reshape(-1)
    rows = np.repeat(np.arange(B), C)
    ok = flat >= 0
    np.add.at(b_dv, flat[ok], d_coef.reshape(-1)[ok, None] * Un[rows[ok]])
    np.add.at(mag, flat[ok], cf.reshape(-1)[ok, None] * Un[rows[ok]])
    b_dv = b_dv + SECOND * gamma(n_j + 1)[:, None] * mag
    return {'parts': (parts, b_parts), 'loss': (float(r['loss'].detach()), float(b_loss)), 'coef': (coef.numpy(), d_coef),
            'dUb': (Ub.grad.numpy(), b_dub), 'dV': (V.grad.numpy(), b_dv), 'scores': (s, ds), 'items': items}


# ---- (d): the order oracle of the item-side gradient ---------------------------------------------------------------------------------------
def fmaf32(a, b, c):
    """round_to_float32(a * b + c) with one rounding, elementwise on float32 arrays"""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b                                                   # exact: 24 + 24 bits
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                             # TwoSum: p + c = s + err exactly
    bits = s.view(np.int64)
    nudge = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(nudge, np.nextafter(s, toward), s)             # round to odd
    return s.astype(np.float32)


def scatter_ordered32(coef32, Ub32, items, n_items, grad=1.0):
    """dV float32 [n_items, D] in the stated order of sbr_scatter_add_scaled_rows_sorted: per item row one fmaf chain from +0 over the slots
    that name it, in ascending slot position (b * C + c); then one float32 multiplication by grad and one addition to +0"""
    B, C = items.shape
    D = Ub32.shape[1]
    acc = np.zeros((n_items, D), dtype=np.float32)
    flat, cf = items.reshape(-1), np.asarray(coef32, dtype=np.float32).reshape(-1)
    for pos in range(B * C):
        j = flat[pos]
        if j >= 0:
            acc[j] = fmaf32(cf[pos], Ub32[pos // C], acc[j])
    return (np.float32(grad) * acc + np.float32(0)).astype(np.float32)


# ---- worlds -------------------------------------------------------------------------------------------------------------------------------
def matrix(n_users, n_items, density, seed, empty_items=(), lonely=True):
    """a 0/1 CSR matrix with the columns ``empty_items`` all zero and, with ``lonely``, one user who alone holds the last two non-empty
    items (their lists have two candidates: shorter than any k > 2)"""
    rng = np.random.default_rng(seed)
    x = (rng.random((n_users, n_items)) < density).astype(np.int8)
    cols = [c for c in range(n_items) if c not in set(empty_items)]
    if lonely:
        x[:, cols[-2:]] = 0
        x[-1, :] = 0
        x[-1, cols[-2:]] = 1
    x[:, list(empty_items)] = 0
    m = sp.csr_matrix(x)
    m.sort_indices()
    return m


def loss_case(D, B, N, K, n_users=23, n_items=19, seed=0, big=True):
    """Operands of one fused-loss case, float32 / int arrays: users repeat, items repeat across rows, some items are positive, negative and
    neighbour at once, lists are shorter than K (lengths 0 .. K), padded slots hold -1, and with ``big`` the first rows are scaled so
    that scores reach about +-30."""
    rng = np.random.default_rng(900 + seed + 7 * D + 11 * B + 13 * N + 17 * K)
    Ut = (rng.standard_normal((n_users, D)) / np.sqrt(D)).astype(np.float32)
    V = rng.standard_normal((n_items, D)).astype(np.float32)
    u = rng.integers(0, min(n_users, max(2, B // 2 + 1)), B).astype(np.int64)
    i = rng.integers(0, n_items, (B, 1 + N)).astype(np.int64)
    i[:, 0] = rng.integers(0, min(n_items, 5), B)                # few positives: they repeat
    if N >= 2:
        i[::2, 1] = i[::2, 0]                                     # the positive is a negative of its own row too
    nbr_len = rng.integers(0, K + 1, n_items).astype(np.int32)
    nbr_len[0], nbr_len[1 % n_items] = K, 0
    nbr_idx = rng.integers(0, n_items, (n_items, K)).astype(np.int32)
    nbr_idx[:, 0] = np.arange(n_items)                            # an item is its own first neighbour
    nbr_val = rng.uniform(0.05, 2., (n_items, K)).astype(np.float32)
    pad = np.arange(K)[None, :] >= nbr_len[:, None]
    nbr_idx[pad], nbr_val[pad] = -1, 0.
    beta_u = rng.uniform(0.1, 1.5, n_users).astype(np.float32)
    beta_u[0] = 0.
    beta_i = rng.uniform(0.05, 1., n_items).astype(np.float32)
    if big:
        Ut[u[0]] = (30. * V[i[0, 0]] / max(float(V[i[0, 0]] @ V[i[0, 0]]), 1e-3)).astype(np.float32)       # s(p) = +30 in row 0
        if B > 1 and u[1] != u[0]:
            Ut[u[1]] = (-30. * V[i[1, 0]] / max(float(V[i[1, 0]] @ V[i[1, 0]]), 1e-3)).astype(np.float32)  # s(p) = -30 in row 1
    return {'Ut': Ut, 'Ub': Ut[u].copy(), 'V': V, 'u': u, 'i': i, 'beta_u': beta_u, 'beta_i': beta_i, 'nbr_idx': nbr_idx, 'nbr_val': nbr_val,
            'nbr_len': nbr_len}


SCALARS = (1e-2, 1.0, 2e-2, 0.7, 30.0, 0.5)                        # every term of the loss at a visible size


def planted_world(seed=0):
    """60 users x 40 items in 4 blocks: a user holds 6 to 9 items of their block and one stray item -> train csr (sorted indices)"""
    rng = np.random.default_rng(4000 + seed)
    x = np.zeros((60, 40), dtype=np.int8)
    for u in range(60):
        blk = u % 4
        x[u, blk * 10 + rng.choice(10, int(rng.integers(6, 10)), replace=False)] = 1
        x[u, rng.integers(0, 40)] = 1
    m = sp.csr_matrix(x)
    m.sort_indices()
    return m


def planted_batches(m, n_batches, B, N, seed=0):
    """[(u [B], i [B, 1 + N])]: observed pairs with N uniform negatives outside the user's row"""
    rng = np.random.default_rng(5000 + seed)
    coo = m.tocoo()
    dense = m.toarray()
    out = []
    for _ in range(n_batches):
        pick = rng.integers(0, coo.nnz, B)
        u, p = coo.row[pick].astype(np.int64), coo.col[pick].astype(np.int64)
        neg = np.empty((B, N), dtype=np.int64)
        for b in range(B):
            neg[b] = rng.choice(np.flatnonzero(dense[u[b]] == 0), N, replace=True)
        out.append((u, np.concatenate([p[:, None], neg], axis=1)))
    return out


def train_torch(m, uw, iw, batches, k, sc, lr, dtype):
    """Adam steps (torch.optim.Adam: betas 0.9 / 0.999, eps 1e-8, no weight decay) of the model in ``dtype`` on the CPU, with the float64
    scales and lists of (a) rounded to float32 once, as the model holds them -> (user table, item table, [loss per step])"""
    bu, bi, row, col = scales32(m)
    nbr_idx, nbr_val, nbr_len = lists32(m, row, col, k)
    U_ = torch.from_numpy(np.asarray(uw, dtype=np.float64)).to(dtype).requires_grad_(True)
    V_ = torch.from_numpy(np.asarray(iw, dtype=np.float64)).to(dtype).requires_grad_(True)
    opt = torch.optim.Adam([U_, V_], lr=lr)
    losses = []
    for u, i in batches:
        opt.zero_grad()
        r = loss_torch(U_[torch.from_numpy(u)], V_, u, i, bu, bi, nbr_idx, nbr_val, nbr_len, sc, dtype)
        r['loss'].backward()
        opt.step()
        losses.append(float(r['loss'].detach()))
    return U_.detach(), V_.detach(), losses


def planted_split(seed=0):
    """planted_world with one block item of every user held out -> (train csr, held int64 [60, 1])"""
    rng = np.random.default_rng(6000 + seed)
    x = planted_world(seed).toarray()
    held = np.zeros((60, 1), dtype=np.int64)
    for u in range(60):
        own = np.flatnonzero(x[u, (u % 4) * 10:(u % 4) * 10 + 10]) + (u % 4) * 10
        held[u, 0] = rng.choice(own)
        x[u, held[u, 0]] = 0
    m = sp.csr_matrix(x)
    m.sort_indices()
    return m, held
