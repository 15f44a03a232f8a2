"""References for SimpleX (csrc/simplex.hip, ``ops.CCLLossFn``, simplex.py). A plain module: no fixtures, no pytest hooks, no GPU. The
definitions are the authors' code as remembered.

(a) Float64 definitions. With nh = max(|H[b]|, eps), nv = max(|V[j]|, eps), y = <H[b], V[j]> / (nh nv) and g = dL/dy (-1/B at the positive,
(negative_weight / N) / B at a negative with y > margin strictly, 0 elsewhere):
    L = mean_b ((1 - y(b, p)) + (negative_weight / N) sum_c max(0, y(b, j_c) - margin))
    coef_a = g / (nh nv)                                   multiplies H[b] in dV[j]
    coef_s = -(g y) / nv^2   (0 where |V[j]| < eps)        multiplies V[j] in dV[j]
    dH[b] = sum_c coef_a V[j_c] - (sum_c g y) / nh^2 H[b]  (the second term 0 where |H[b]| < eps)
A slot whose index lies outside [0, n_items) has y = 0, both coefficients 0 and adds no term. ``loss_torch`` is the plain torch composition
(gather, clamp, relu, autograd), ``direct`` the formulas above in numpy; the CPU tests hold them against each other and against central
finite differences. eps, margin and negative_weight are the float32 numbers the kernel receives, taken as exact.

(b) The float32 restatement of both kernels in the exact order of include/sibrar_hip.h: ``ccl32`` and ``scatter_cos32``, numpy float32
operations (numpy never fuses; ``fmaf32`` is the correctly rounded fused operation, tests/ultragcn_ref.py (d) restated here because no test
module imports another's reference).

(c) The bound of the fused loss, derived from that order, never fitted. u = 2^-24, SECOND = 1.01 for second-order terms, gamma(t) = t u /
(1 - t u). sqrtf and the divisions are taken at 2 u although they are correctly rounded. Per slot, A = sum_d |H_d V_d|:
    s, hh, vv   a dot product of D terms, however the chain and the butterfly split it: gamma(D) A, gamma(D) hh, gamma(D) vv
    nh, nv      the square root halves the relative error, then its own rounding: rn = gamma(D) / 2 + 2 u; max(., eps) is 1-Lipschitz
    den         = nh * nv: rd = 2 rn + u
    y           = s / den:  dy <= gamma(D) A / den + (rd + 2 u) |y|
    g           fl(1 / B) 2 u; fl(negative_weight / N) 2 u on a float32 numerator, the product one more: 6 u taken for both kinds
    coef_a      = g / den:  (6 u + rd + 2 u) |coef_a|
    gy          = g * y:    d gy <= |g| dy + 7 u |gy|
    coef_s      = -(gy / (nv * nv)):  d gy / nv^2 + (2 rn + u + 2 u) |coef_s|
    sgy         N additions of 1 + N terms:  sum d gy + gamma(N) sum |gy|
    k           = sgy / (nh * nh):  d sgy / nh^2 + (2 rn + 3 u) sum |gy| / nh^2
    dH[d]       a chain of 1 + N fmaf and one more:  sum_c d coef_a |V_cd| + dk |H_d| + gamma(N + 2) (sum_c |coef_a V_cd| + (sum |gy| / nh^2) |H_d|)
    terms       1 - y and max(y - margin, 0): dy + u |term|; summed in double; each part rounded once (+ u |part|)
    dV[j, d]    S a chain over the n_j slots that name j, T a sum over the same, r = fmaf(T, V, S), the product with grad, the addition to
                dst:  sum d coef_a |H_d| + |V_jd| (sum d coef_s + gamma(n_j) sum |coef_s|) + gamma(n_j + 3) (sum |coef_a H_d| + |V_jd| sum |coef_s|)
The bound assumes that the hinge's active set is the reference's: every input set of the GPU tests keeps |y - margin| >= 1e-3 at every
negative slot (``margin_gap``; tests/test_simplex_cpu.py checks it on the float64 scores), far above dy, or holds scores that equal the
margin exactly in both precisions (``margin_cases``)."""
import numpy as np
import scipy.sparse as sp
import torch

U = 2.0 ** -24
SECOND = 1.01
# The one tolerance here that is not the derived bound: the whole-model tests (tests/test_hip_simplex.py) pass through the pooling, the D x D
# map, the lookup and torch's elementwise mix besides the loss, whose bounds are pinned in their own test modules and are not composed here.
# Those tests allow FACTOR times the largest error of the same network in torch float32 on the CPU against float64, the yardstick and the
# multiple of tests/ultragcn_ref.py. The kernel tests (tests/test_hip_ccl_loss.py) use the derived bound of (c) alone.
FACTOR = 8.0
EPS = float(np.float32(1e-8))             # ops.COS_EPS as the kernel receives it
GAP = 1e-3


def gamma(t):
    t = np.asarray(t, dtype=np.float64)
    return t * U / (1 - t * U)


def f32(x):
    return float(np.float32(x))


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------
def loss_torch(H, V, i_idx, margin, negw, eps=EPS):
    """the torch composition in the dtype of H: (L, pos, neg, y [B, 1 + N]); slots outside the table are masked out"""
    i_idx = torch.as_tensor(np.asarray(i_idx), dtype=torch.int64)
    B, C = i_idx.shape
    N = C - 1
    valid = (i_idx >= 0) & (i_idx < V.shape[0])
    rows = V[torch.where(valid, i_idx, torch.zeros_like(i_idx))]
    nh = H.norm(dim=1).clamp(min=eps)
    nv = rows.norm(dim=2).clamp(min=eps)
    y = torch.einsum('bd,bcd->bc', H, rows) / (nh[:, None] * nv) * valid
    pos = ((1 - y[:, 0]) * valid[:, 0]).sum() / B
    neg = (torch.relu(y[:, 1:] - margin) * valid[:, 1:]).sum() / N / B
    return pos + negw * neg, pos, neg, y


def direct(H, V, i_idx, margin, negw, eps=EPS):
    """the formulas of (a) in float64 numpy -> dict"""
    H, V = np.asarray(H, dtype=np.float64), np.asarray(V, dtype=np.float64)
    i_idx = np.asarray(i_idx, dtype=np.int64)
    B, C = i_idx.shape
    N, n_items = C - 1, V.shape[0]
    valid = (i_idx >= 0) & (i_idx < n_items)
    safe = np.where(valid, i_idx, 0)
    Vs = V[safe] * valid[:, :, None]
    rh = np.sqrt((H * H).sum(1))
    rv = np.sqrt((Vs * Vs).sum(2))
    nh, nv = np.maximum(rh, eps), np.maximum(rv, eps)
    den = nh[:, None] * nv
    y = np.einsum('bd,bcd->bc', H, Vs) / den * valid
    g = np.zeros((B, C))
    g[:, 0] = -1. / B
    g[:, 1:] = (negw / N / B) * (y[:, 1:] > margin)
    g = g * valid
    ca = g / den
    cs = np.where(rv < eps, 0., -(g * y) / (nv * nv))
    sgy_abs = np.abs(g * y).sum(1)
    k = np.where(rh < eps, 0., (g * y).sum(1) / (nh * nh))
    dH = np.einsum('bc,bcd->bd', ca, Vs) - k[:, None] * H
    dV = np.zeros_like(V)
    np.add.at(dV, safe[valid], (ca[:, :, None] * H[:, None, :] + cs[:, :, None] * Vs)[valid])
    pos = ((1 - y[:, 0]) * valid[:, 0]).sum() / B
    neg = (np.maximum(y[:, 1:] - margin, 0.) * valid[:, 1:]).sum() / N / B
    return {'y': y, 'g': g, 'coef_a': ca, 'coef_s': cs, 'dH': dH, 'dV': dV, 'pos': pos, 'neg': neg, 'loss': pos + negw * neg, 'valid': valid,
            'safe': safe, 'Vs': Vs, 'rh': rh, 'rv': rv, 'nh': nh, 'nv': nv, 'den': den, 'k_abs': sgy_abs / (nh * nh)}


def margin_gap(H, V, i_idx, margin):
    """the smallest |y - margin| over the negative slots inside the table, in float64 on the float32 inputs"""
    r = direct(H, V, i_idx, f32(margin), 1.)
    d = np.abs(r['y'][:, 1:] - f32(margin))[r['valid'][:, 1:]]
    return float(d.min()) if d.size else np.inf


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------
def reference(H32, V32, i_idx, margin, negw, eps=EPS):
    """Everything the kernel tests compare against, in float64 on the float32 inputs, with the bounds of (c): (value, bound) pairs for
    'parts' [3] = (pos, neg, L), 'scores', 'coef_a', 'coef_s', 'dH', 'dV'; plus 'r', the dict of ``direct``"""
    margin, negw = f32(margin), f32(negw)
    r = direct(H32, V32, i_idx, margin, negw, eps)
    H, V = np.abs(np.asarray(H32, dtype=np.float64)), np.abs(np.asarray(V32, dtype=np.float64))
    B, C = r['y'].shape
    N, D, n_items = C - 1, H.shape[1], V.shape[0]
    valid, Vs = r['valid'], np.abs(r['Vs'])
    gD = float(gamma(D))
    rn = gD / 2 + 2 * U
    rd = 2 * rn + U
    A = np.einsum('bd,bcd->bc', H, Vs)
    y, g, ca, cs = r['y'], np.abs(r['g']), np.abs(r['coef_a']), np.abs(r['coef_s'])
    dy = SECOND * (gD * A / r['den'] + (rd + 2 * U) * np.abs(y)) * valid
    d_ca = SECOND * (8 * U + rd) * ca
    gy = g * np.abs(y)
    d_gy = SECOND * (g * dy + 7 * U * gy)
    d_cs = SECOND * np.where(r['rv'] < eps, 0., d_gy / r['nv'] ** 2 + (2 * rn + 3 * U) * cs)
    d_sgy = d_gy.sum(1) + SECOND * gamma(N) * gy.sum(1)
    live = r['rh'] >= eps
    dk = SECOND * np.where(live, d_sgy / r['nh'] ** 2 + (2 * rn + 3 * U) * r['k_abs'], 0.)
    k_abs = np.where(live, r['k_abs'], 0.)
    b_dH = np.einsum('bc,bcd->bd', d_ca, Vs) + dk[:, None] * H + SECOND * gamma(N + 2) * (np.einsum('bc,bcd->bd', ca, Vs) + k_abs[:, None] * H)
    t_pos = np.abs(1 - y[:, 0]) * valid[:, 0]
    t_neg = np.maximum(y[:, 1:] - margin, 0.) * valid[:, 1:]
    raw_pos = ((dy[:, 0] + U * t_pos) * valid[:, 0]).sum() / B
    raw_neg = ((dy[:, 1:] + U * t_neg) * (t_neg > 0)).sum() / N / B
    parts = np.array([r['pos'], r['neg'], r['loss']])
    b_parts = SECOND * np.array([raw_pos, raw_neg, raw_pos + negw * raw_neg]) + 2 * U * np.abs(parts)
    n_j = np.bincount(r['safe'][valid], minlength=n_items).astype(np.float64)
    acc = {k: np.zeros((n_items, D)) for k in ('dca', 'ca')}
    col = {k: np.zeros(n_items) for k in ('dcs', 'cs')}
    Hb = np.broadcast_to(H[:, None, :], (B, C, D))
    np.add.at(acc['dca'], r['safe'][valid], (d_ca[:, :, None] * Hb)[valid])
    np.add.at(acc['ca'], r['safe'][valid], (ca[:, :, None] * Hb)[valid])
    np.add.at(col['dcs'], r['safe'][valid], d_cs[valid])
    np.add.at(col['cs'], r['safe'][valid], cs[valid])
    b_dV = acc['dca'] + V * (col['dcs'] + SECOND * gamma(n_j) * col['cs'])[:, None] \
        + SECOND * gamma(n_j + 3)[:, None] * (acc['ca'] + V * col['cs'][:, None])
    return {'parts': (parts, b_parts), 'scores': (y, dy), 'coef_a': (r['coef_a'], d_ca), 'coef_s': (r['coef_s'], d_cs), 'dH': (r['dH'], b_dH),
            'dV': (r['dV'], b_dV), 'r': r}


def worst_ratios(got, ref, keys=('parts', 'scores', 'coef_a', 'coef_s', 'dH', 'dV')):
    """{key: max |got - want| / bound} (0 where the error is 0; NaN in ``got`` gives inf)"""
    out = {}
    for k in keys:
        want, bound = ref[k]
        err = np.abs(np.asarray(got[k], dtype=np.float64) - want)
        err = np.where(np.isnan(err), np.inf, err)
        out[k] = float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.)))
    return out


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------
def fmaf32(a, b, c):
    """round_to_float32(a * b + c) with one rounding, elementwise on float32 arrays: the product is exact in float64, the sum is rounded
    to odd in float64 (TwoSum gives the error term) and then to nearest float32 (53 >= 2 * 24 + 2)"""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64)
    nudge = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    s = np.where(nudge, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def geometry(D):
    """(V, G, C): columns per chunk, lanes per group, chunks per lane"""
    Vw = 4 if D % 4 == 0 else 1
    chunks = D // Vw
    G = 1
    while G < 64 and G < chunks:
        G *= 2
    return Vw, G, -(-chunks // G)


def group_dot32(a, b):
    """<a, b> per row of two float32 arrays [..., D] in the kernel's order: lane l of the G lanes chains its columns in ascending order
    from +0, then the xor butterfly from offset G / 2 down to 1"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    D = a.shape[-1]
    Vw, G, C = geometry(D)
    lanes = np.zeros(a.shape[:-1] + (G,), dtype=np.float32)
    for l in range(G):
        for k in range(C):
            for j in range(Vw):
                col = (l + k * G) * Vw + j
                if col < D:
                    lanes[..., l] = fmaf32(a[..., col], b[..., col], lanes[..., l])
    off = G // 2
    while off > 0:
        lanes = (lanes + lanes[..., np.arange(G) ^ off]).astype(np.float32)
        off //= 2
    return lanes[..., 0]


def ccl32(H32, V32, i_idx, margin, negw, eps=EPS):
    """sbr_ccl_loss_fwd_bwd in numpy float32, operation by operation -> dict of float32 arrays ('parts' [3], 'scores', 'coef_a', 'coef_s', 'dH')"""
    F = np.float32
    H32, V32 = np.asarray(H32, dtype=F), np.asarray(V32, dtype=F)
    i_idx = np.asarray(i_idx, dtype=np.int64)
    B, C = i_idx.shape
    N, D, n_items = C - 1, H32.shape[1], V32.shape[0]
    margin, eps = F(margin), F(eps)
    inv_b = F(1) / F(B)
    g_pos, g_neg = -inv_b, (F(negw) / F(N)) * inv_b
    valid = (i_idx >= 0) & (i_idx < n_items)
    rows = V32[np.where(valid, i_idx, 0)]
    rh = np.sqrt(group_dot32(H32, H32))
    nh = np.maximum(rh, eps)
    s = group_dot32(np.broadcast_to(H32[:, None, :], rows.shape), rows)
    rv = np.sqrt(group_dot32(rows, rows))
    nv = np.maximum(rv, eps)
    den = (nh[:, None] * nv).astype(F)
    with np.errstate(invalid='ignore', divide='ignore'):
        y = np.where(valid, (s / den).astype(F), F(0))
        g = np.where(np.arange(C)[None, :] == 0, g_pos, np.where(y > margin, g_neg, F(0))).astype(F)
        g = np.where(valid, g, F(0))
        on = g != 0
        ca = np.where(on, (g / den).astype(F), F(0))
        gy = (g * y).astype(F)
        cs = np.where(on & ~(rv < eps), -(gy / (nv * nv).astype(F)).astype(F), F(0))
    sgy, acc = np.zeros(B, dtype=F), np.zeros((B, D), dtype=F)
    pos, neg = np.zeros(B), np.zeros(B)
    for c in range(C):
        sgy = np.where(on[:, c], (sgy + gy[:, c]).astype(F), sgy)
        acc = np.where(on[:, c, None], fmaf32(ca[:, c, None], rows[:, c], acc), acc)
        if c == 0:
            pos += np.where(valid[:, 0], (F(1) - y[:, 0]).astype(F), F(0)).astype(np.float64)
        else:
            neg += np.where(valid[:, c], np.maximum((y[:, c] - margin).astype(F), F(0)), F(0)).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        k = np.where(rh < eps, F(0), (sgy / (nh * nh).astype(F)).astype(F))
    dH = fmaf32(-k[:, None], H32, acc)
    row_parts = np.stack([pos, neg / N], axis=1)
    lanes = np.zeros((64, 2))
    for b in range(B):
        lanes[b % 64] += row_parts[b]
    off = 32
    while off > 0:
        lanes = lanes + lanes[np.arange(64) ^ off]
        off //= 2
    p, n = lanes[0]
    parts = np.array([p / B, n / B, (p + float(F(negw)) * n) / B]).astype(F)
    return {'parts': parts, 'scores': y, 'coef_a': ca, 'coef_s': cs, 'dH': dH}


def scatter_cos32(ca32, cs32, H32, V32, i_idx, grad=1.0, dst=None):
    """sbr_scatter_add_cos_rows_sorted in numpy float32: per table row S (a fmaf chain) and T (a sum) over the slots that name it, in
    ascending slot position; r = fmaf(T, V, S); dst += grad * r. Rows that no slot names keep the contents of ``dst`` (zeros by default)"""
    F = np.float32
    i_idx = np.asarray(i_idx, dtype=np.int64)
    B, C = i_idx.shape
    n_items, D = V32.shape
    S, T = np.zeros((n_items, D), dtype=F), np.zeros(n_items, dtype=F)
    named = np.zeros(n_items, dtype=bool)
    flat, a, s = i_idx.reshape(-1), np.asarray(ca32, dtype=F).reshape(-1), np.asarray(cs32, dtype=F).reshape(-1)
    for pos in range(B * C):
        j = flat[pos]
        if 0 <= j < n_items:
            S[j] = fmaf32(a[pos], H32[pos // C], S[j])
            T[j] = T[j] + s[pos]
            named[j] = True
    out = np.zeros((n_items, D), dtype=F) if dst is None else np.array(dst, dtype=F)
    t = (F(grad) * fmaf32(T[:, None], V32, S)).astype(F)
    out[named] = (out[named] + t[named]).astype(F)
    return out


# ---- input sets of the GPU tests (tests/test_hip_ccl_loss.py); tests/test_simplex_cpu.py checks margin_gap on each -----------------------------
def _dims():
    out = []
    for n, D in enumerate((1, 3, 4, 64, 68, 256)):
        pairs = ((1, 1), (5, 2), (33, 65), (5, 130)) if n % 2 == 0 else ((33, 1), (1, 2), (5, 65), (33, 130))
        out += [(D, N, B) for N, B in pairs]
    return out


SHAPE_CASES = _dims()                      # (D, N, B): every D, N and B of the issue; both chunk widths at one and several rows per wave
SLOT_CASES = ('repeats', 'outside', 'zero_rows')


def shape_case(D, N, B):
    """-> (H, V, i, margin, negative_weight). The cosines of random rows are spread round 0 (for D = 1 every one is +-1), so a margin
    near 0 leaves active and inactive negatives at every D. The margin is moved up from 0 in steps of 1 / 64 until no negative's score
    lies within GAP of it: a function of the reference alone."""
    rng = np.random.default_rng(70000 + 1000 * D + 10 * N + B)
    n_items = 7 + (D + N + B) % 44
    H = rng.standard_normal((B, D)).astype(np.float32)
    V = (rng.standard_normal((n_items, D)) * rng.uniform(0.2, 3., (n_items, 1))).astype(np.float32)
    i = rng.integers(0, n_items, (B, 1 + N)).astype(np.int64)
    margin = 0.0
    while margin_gap(H, V, i, margin) < GAP:
        margin += 1. / 64
    return H, V, i, margin, 2.5


def slot_case(kind):
    rng = np.random.default_rng(80000 + SLOT_CASES.index(kind))
    B, N, D, n_items = 9, 6, 12, 11
    H = rng.standard_normal((B, D)).astype(np.float32)
    V = rng.standard_normal((n_items, D)).astype(np.float32)
    i = rng.integers(0, n_items, (B, 1 + N)).astype(np.int64)
    if kind == 'repeats':
        i[0, 1:] = i[0, 1]                                        # one item in every negative slot of row 0
        i[:, 2] = i[:, 0]                                         # the positive is a negative of its own row too
        i[:, 4] = i[:, 3]                                         # an item repeated within a row
    elif kind == 'outside':
        i[::2, 1], i[1::2, 3] = -1, n_items                       # these read nothing
        i[3, 0], i[4, 0] = -1, n_items                            # also as the positive
    else:
        V[2], V[5], H[1], H[6] = 0., 0., 0., 0.
        i[0, 0], i[1, 0], i[2, 1], i[6, 2] = 2, 5, 2, 5           # a zero item row as positive and as negative, under a zero H row too
    margin = -0.25                                                 # below 0: a score of exactly 0 is active
    while margin_gap(H, V, i, margin) < GAP:
        margin -= 1. / 64
    return H, V, i, margin, 3.0


def margin_cases():
    """[(name, H, V, i, margin, negative_weight, all negatives active?)]: an all-identical table of rows (1/2, 1/2, 1/2, 1/2) under
    margin = 1, where the rows of H that are parallel to it score exactly 1 in float32 and in float64 (hh = vv = s = 1, every operation
    exact) and nothing is active; and a generic table under margin = -1, where everything is active"""
    rng = np.random.default_rng(90000)
    B, N, D, n_items = 6, 5, 4, 8
    V = np.full((n_items, D), 0.5, dtype=np.float32)
    H = rng.standard_normal((B, D)).astype(np.float32)
    H[0], H[3] = 0.5, 0.5
    i = rng.integers(0, n_items, (B, 1 + N)).astype(np.int64)
    V2 = rng.standard_normal((n_items, D)).astype(np.float32)
    return [('identical table, margin 1', H, V, i, 1.0, 2.0, False), ('margin -1', H, V2, i, -1.0, 2.0, True)]


# ---- the whole model ----------------------------------------------------------------------------------------------------------------------
def world(seed=0):
    """a 0/1 CSR matrix of 40 users x 30 items; user 7 has an empty history, user 8 a single item"""
    rng = np.random.default_rng(3000 + seed)
    x = (rng.random((40, 30)) < 0.2).astype(np.int8)
    x[7] = 0
    x[8] = 0
    x[8, 4] = 1
    m = sp.csr_matrix(x)
    m.sort_indices()
    return m


def history32(m):
    """the dense users x items matrix of 1 / d_u rounded to float32 once, as the model holds it (0 where d_u = 0)"""
    x = (m.toarray() != 0)
    deg = x.sum(1)
    return x * (1. / np.maximum(deg, 1)).astype(np.float32)[:, None]


def model_loss(m, Uw, Vw, W, u, i, gamma_, margin, negw, dtype=torch.float64):
    """the model's forward pass in ``dtype`` by the torch composition; Uw, Vw, W: torch leaves -> (L, pos, neg, y, h)"""
    P = torch.from_numpy(np.asarray(history32(m), dtype=np.float64)).to(dtype)
    u = torch.as_tensor(np.asarray(u), dtype=torch.int64)
    h = gamma_ * Uw[u] + (1. - gamma_) * ((P[u] @ Vw) @ W.t())
    return loss_torch(h, Vw, i, f32(margin), f32(negw)) + (h,)


def batches(m, n_batches, B, N, seed=0):
    """[(u [B], i [B, 1 + N])]: observed pairs (the user without history appears through a planted row) with N uniform negatives"""
    rng = np.random.default_rng(5000 + seed)
    coo = m.tocoo()
    out = []
    for _ in range(n_batches):
        pick = rng.integers(0, coo.nnz, B)
        u, p = coo.row[pick].astype(np.int64), coo.col[pick].astype(np.int64)
        u[0], p[0] = 7, 3                                         # the user with the empty history
        neg = rng.integers(0, m.shape[1], (B, N)).astype(np.int64)
        out.append((u, np.concatenate([p[:, None], neg], axis=1)))
    return out


MODEL_GAMMAS = (0.0, 0.5, 1.0)


def model_case(gamma_, D=8, B=24, N=6):
    """One training batch of the whole model on ``world()`` -> dict(m, U, V, W float32 arrays, u, i, gamma, margin, negative_weight); the
    margin is moved in steps of 1 / 64 until no negative of the float64 model scores within GAP of it"""
    rng = np.random.default_rng(6000 + int(100 * gamma_))
    m = world()
    Uw = (rng.standard_normal((40, D)) * 0.5).astype(np.float32)
    Vw = (rng.standard_normal((30, D)) * 0.5).astype(np.float32)
    W = (rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)
    u, i = batches(m, 1, B, N, seed=int(100 * gamma_))[0]
    t = lambda a: torch.from_numpy(a.astype(np.float64))
    margin = 0.125
    while True:
        h = model_loss(m, t(Uw), t(Vw), t(W), u, i, gamma_, margin, 1.)[4].numpy()
        if margin_gap(h, Vw, i, margin) >= GAP:
            break
        margin += 1. / 64
    return {'m': m, 'U': Uw, 'V': Vw, 'W': W, 'u': u, 'i': i, 'gamma': gamma_, 'margin': margin, 'negative_weight': 4.0}


def model_grads(c, dtype):
    """(L, y, h, {parameter: gradient}) of ``model_case`` c by torch autograd in ``dtype`` on the CPU"""
    leaves = {k: torch.from_numpy(c[k].astype(np.float64)).to(dtype).requires_grad_(True) for k in ('U', 'V', 'W')}
    L, pos, neg, y, h = model_loss(c['m'], leaves['U'], leaves['V'], leaves['W'], c['u'], c['i'], c['gamma'], c['margin'], c['negative_weight'],
                                   dtype)
    L.backward()
    return float(L.detach()), y.detach(), h.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
