"""References for the multinomial likelihood kernel (csrc/multinomial.hip, ``ops.multinomial_nll``, ``ops.MultinomialNLLFn``) and the
Mult-VAE / Mult-DAE models (multvae.py), and the planted world their tests share. A plain module: numpy and torch on the CPU, no
fixtures, no GPU.

Definitions (float64), for a logit row z of n_items values and a user's set S of n items:
  lse = log sum_j exp(z_j);  row_loss = n lse - sum_{i in S} z_i;  d_j = gs (n exp(z_j - lse) - [j in S]);  n == 0: zero loss, zero row.

Error bound of ``sbr_multinomial_nll_f32`` against float64 on the same fp32 inputs, from the geometry stated in include/sibrar_hip.h.
u = 2^-24. E_EXP and E_LOG are the relative errors allowed for one expf / logf call of the device library (measured, see below). T is
the number of threads that own a row (64 up to n_items = 1024, 256 above), C = ceil(ceil(n_items / 4) / T) the chunks of one thread,
M = max_j z_j (exact: a maximum does not round), a_j = M - z_j >= 0 and s = sum_j exp(-a_j) >= 1.
  The term of element j enters its thread's sum as expf(fl(z_j - m')) with m' the running maximum, and is then multiplied by
  e(m', m''), e(m'', m'''), ... up to M: at most C - 1 more factors in the thread, 6 in the butterfly and 3 across the waves. The
  arguments of all these exponentials are differences of a monotone chain from z_j up to M, so their absolute values add up to a_j, and
  their roundings shift the exponent by at most u a_j (1 + u) in total. That makes K = C + 10 expf calls with relative error E_EXP each,
  N = 5 C + 18 roundings of products and sums (4 C additions and C products in the thread, 9 of each in the merges), and one factor
  exp(t), |t| <= 1.01 u a_j. With X_j = K E_EXP + N u + 1.01 u a_j, the computed sum is sum_j exp(-a_j) (1 + q_j), |q_j| <= X_j / (1 - X_j):
      err_s = sum_j exp(-a_j) X_j / (1 - X_j) + n_items K 2^-126      (the last term: results that underflow)
  lse = fl(M + logf(s^)): with r = err_s / s,
      err_log = (|log s| + r) E_LOG + r / (1 - r);   err_lse = err_log + u (|lse| + err_log).
  pos: a thread adds ceil(n / T) entries, then 9 merges: err_pos = gamma(ceil(n / T) + 9) sum_{i in S} |z_i|.
  row_loss = fl(fl(n lse^) - pos^): err_a = n err_lse + u (n |lse| + n err_lse);
      err_loss = err_a + err_pos + u (|n lse - pos| + err_a + err_pos).
  d_j (dense part) = fl(gs fl(n expf(fl(z_j - lse^)))): the exponent is off by at most err_lse + 1.01 u (|z_j - lse| + err_lse), then one
  expf and two products: with Y_j = err_lse + 1.01 u (|z_j - lse| + err_lse) + E_EXP + 2 u,
      err_d_j = |gs| n (exp(z_j - lse) Y_j / (1 - Y_j) + 2^-126), and at the positives + u (|d_j| + err_d_j) for the subtraction.
  A gradient row sums to zero exactly, so |sum_j d^_j| <= sum_j err_d_j.

E_EXP and E_LOG: ROCm's math documentation is not installed beside the compiler, so the largest error of the device's expf over
[-104, 0] and of logf over [1, 2^21] was measured once against float64 on an MI355X (DESIGN.md §4.30 has the figures and the date);
the constants are twice the measured ulps, one ulp taken as a relative 2^-23."""
import numpy as np
import scipy.sparse as sp
import torch

U = 2.0 ** -24
EXPF_ULPS = 2.0            # twice the largest measured error of expf, in ulps: 1.00
LOGF_ULPS = 4.6            # the same for logf: 2.30
E_EXP = EXPF_ULPS * 2.0 ** -23
E_LOG = LOGF_ULPS * 2.0 ** -23
TINY = 2.0 ** -126
WAVE_MAX, STAGE_MAX = 1024, 12288          # csrc/multinomial.hip: MN_WAVE_MAX, MN_STAGE_MAX


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1 - k * U)


def threads(n_items):
    return 64 if n_items <= WAVE_MAX else 256


# ---- the loss ---------------------------------------------------------------------------------------------------------------------------
def nll64(z, targets, gs=None):
    """z [B, I] (any float dtype), targets [B, I] 0/1 -> (row_loss, row_lse, d or None) in float64"""
    z = np.asarray(z, dtype=np.float64)
    t = np.asarray(targets, dtype=np.float64)
    m = z.max(1, keepdims=True)
    lse = (m + np.log(np.exp(z - m).sum(1, keepdims=True)))[:, 0]
    n = t.sum(1)
    loss = np.where(n > 0, n * lse - (z * t).sum(1), 0.0)
    d = None if gs is None else float(gs) * (n[:, None] * np.exp(z - lse[:, None]) - t)
    return loss, lse, d


def nll_bound(z, targets, gs=None):
    """-> (err_loss [B], err_lse [B], err_d [B, I] or None): the bounds of the module docstring, float64"""
    z = np.asarray(z, dtype=np.float64)
    t = np.asarray(targets, dtype=np.float64)
    B, I = z.shape
    T = threads(I)
    C = -(-(-(-I // 4)) // T)
    K, N = C + 10, 5 * C + 18
    M = z.max(1, keepdims=True)
    a = M - z
    ea = np.exp(-a)
    s = ea.sum(1)
    X = K * E_EXP + N * U + 1.01 * U * a
    assert float(X.max()) < 0.5
    err_s = (ea * X / (1 - X)).sum(1) + I * K * TINY
    r = err_s / s
    lse = M[:, 0] + np.log(s)
    err_log = (np.abs(np.log(s)) + r) * E_LOG + r / (1 - r)
    err_lse = err_log + U * (np.abs(lse) + err_log)
    n = t.sum(1)
    err_pos = gamma(np.ceil(n / T) + 9) * (np.abs(z) * t).sum(1)
    err_a = n * err_lse + U * (n * np.abs(lse) + n * err_lse)
    pos = (z * t).sum(1)
    err_loss = np.where(n > 0, err_a + err_pos + U * (np.abs(n * lse - pos) + err_a + err_pos), 0.0)
    if gs is None:
        return err_loss, err_lse, None
    g = abs(float(gs))
    zl = z - lse[:, None]
    Y = err_lse[:, None] + 1.01 * U * (np.abs(zl) + err_lse[:, None]) + E_EXP + 2 * U
    assert float(Y.max()) < 0.5
    err_d = g * n[:, None] * (np.exp(zl) * Y / (1 - Y) + TINY)
    d = g * np.abs(n[:, None] * np.exp(zl) - t)
    err_d = err_d + t * U * (d + err_d)
    return err_loss, err_lse, err_d


def coarse_row_sum_bound(n_items, n, zmax, zmin, lse, gs):
    """An upper bound of sum_j err_d_j of ``nll_bound`` from a row's extremes alone (float64 arrays [B]): every X_j and Y_j is replaced
    by its largest possible value (a_j <= zmax - zmin, |z_j - lse| <= max(lse - zmin, |zmax - lse|)) and sum_j exp(z_j - lse) = 1."""
    T = threads(n_items)
    C = -(-(-(-n_items // 4)) // T)
    K, N = C + 10, 5 * C + 18
    X = K * E_EXP + N * U + 1.01 * U * (zmax - zmin)
    r = X / (1 - X) + n_items * K * TINY
    err_log = (np.abs(lse - zmax) + r) * E_LOG + r / (1 - r)
    err_lse = err_log + U * (np.abs(lse) + err_log)
    Y = err_lse + 1.01 * U * (np.maximum(lse - zmin, np.abs(zmax - lse)) + err_lse) + E_EXP + 2 * U
    g = abs(float(gs))
    dense = g * n * (Y / (1 - Y) + n_items * TINY)
    return dense + n * U * (g * np.maximum(n, 1) + dense)              # at a positive |d_j| = g |n p_j - 1| <= g max(n, 1)


# ---- the float64 model ------------------------------------------------------------------------------------------------------------------
PARAMS = ('w_enc1', 'b_enc1', 'w_enc2', 'b_enc2', 'w_dec1', 'b_dec1', 'w_dec2', 'b_dec2')


def init_params(n_items, hidden, latent, variational, seed, dtype=torch.float64):
    """Xavier-normal weights, biases normal with std 0.001, the package's parameter names"""
    g = torch.Generator().manual_seed(int(seed))
    code = 2 * latent if variational else latent
    p = {}
    for name, (out, inp) in zip(('enc1', 'enc2', 'dec1', 'dec2'), ((hidden, n_items), (code, hidden), (hidden, latent), (n_items, hidden))):
        p['w_' + name] = (torch.randn(out, inp, generator=g, dtype=torch.float64) * (2.0 / (out + inp)) ** 0.5).to(dtype).requires_grad_()
        p['b_' + name] = (torch.randn(out, generator=g, dtype=torch.float64) * 0.001).to(dtype).requires_grad_()
    return p


def normalised_rows(x):
    """x [B, I] 0/1 -> the rows divided by max(||row||_2, 1e-8)"""
    return x / x.pow(2).sum(1, keepdim=True).sqrt().clamp(min=1e-8)


def forward(p, x, variational, eps=None, keep=None, dropout=0.0, beta=0.0):
    """The model in torch, in the dtype of the parameters. x [B, I]: the 0/1 rows (also the targets); keep [B, I]: the dropout keep-mask
    (None: no dropout), applied to the normalised rows with the scale 1 / (1 - dropout); eps [B, latent]: the noise (None: z = mu).
    -> (loss, nll, kl, logits)"""
    dt = p['w_enc1'].dtype
    x = x.to(dt)
    h = normalised_rows(x)
    if keep is not None:
        h = h * keep.to(dt) / (1.0 - dropout)
    h = torch.tanh(h @ p['w_enc1'].t() + p['b_enc1'])
    e = h @ p['w_enc2'].t() + p['b_enc2']
    kl = None
    if variational:
        latent = e.shape[1] // 2
        mu, logvar = e[:, :latent], e[:, latent:]
        z = mu if eps is None else mu + eps.to(dt) * torch.exp(0.5 * logvar)
        kl = 0.5 * (-logvar + torch.exp(logvar) + mu * mu - 1).sum(1).mean()
    else:
        z = torch.tanh(e)
    logits = torch.tanh(z @ p['w_dec1'].t() + p['b_dec1']) @ p['w_dec2'].t() + p['b_dec2']
    n = x.sum(1)
    row = n * torch.logsumexp(logits, 1) - (logits * x).sum(1)
    nll = torch.where(n > 0, row, torch.zeros_like(row)).mean()
    return (nll + beta * kl if variational else nll), nll, kl, logits


# ---- the planted world ------------------------------------------------------------------------------------------------------------------
N_USERS, N_ITEMS, N_BLOCKS, PER_USER, HELD_OUT = 240, 96, 4, 10, 2
SETTINGS = dict(hidden=32, latent=8, batch_size=60, lr=1e-2, dropout=0.5, anneal_cap=0.2, total_anneal_steps=100, n_epochs=40)


def planted_world(seed=0):
    """240 users x 96 items in 4 blocks; a user has 10 items of their block, 2 of them held out -> (train csr, held out int64 [240, 2])"""
    rng = np.random.default_rng(1000 + seed)
    ub, ib = N_USERS // N_BLOCKS, N_ITEMS // N_BLOCKS
    rows, cols, held = [], [], np.zeros((N_USERS, HELD_OUT), dtype=np.int64)
    for u in range(N_USERS):
        items = (u // ub) * ib + rng.choice(ib, size=PER_USER, replace=False)
        held[u] = items[:HELD_OUT]
        rows += [u] * (PER_USER - HELD_OUT)
        cols += list(items[HELD_OUT:])
    train = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(N_USERS, N_ITEMS))
    train.sort_indices()
    return train, held


def ndcg_at_10(scores, train, held):
    """scores [U, I] (numpy); the training items are excluded; mean NDCG@10 of the held-out items"""
    s = np.array(scores, dtype=np.float64)
    s[train.nonzero()] = -np.inf
    top = np.argsort(-s, axis=1, kind='stable')[:, :10]
    disc = 1.0 / np.log2(np.arange(10) + 2)
    ideal = disc[:held.shape[1]].sum()
    hit = (top[:, :, None] == held[:, None, :]).any(2)
    return float(((hit * disc).sum(1) / ideal).mean())


def popularity_scores(train):
    return np.tile(np.asarray(train.sum(0)).reshape(1, -1), (train.shape[0], 1))


def train_reference(train, variational, seed, hidden, latent, batch_size, lr, dropout, anneal_cap, total_anneal_steps, n_epochs):
    """The float64 model trained with torch's Adam as fit() trains the package's -> the score rows [U, I] (z = mu, no dropout)"""
    x_all = torch.from_numpy(np.asarray(train.todense(), dtype=np.float64))
    p = init_params(train.shape[1], hidden, latent, variational, seed)
    opt = torch.optim.Adam(list(p.values()), lr=lr)
    g = torch.Generator().manual_seed(int(seed))
    active = torch.nonzero(x_all.sum(1) > 0).reshape(-1)
    step = 0
    for _ in range(n_epochs):
        order = active[torch.randperm(active.numel(), generator=g)]
        for lo in range(0, order.numel(), batch_size):
            x = x_all[order[lo:lo + batch_size]]
            beta = min(anneal_cap, anneal_cap * step / total_anneal_steps)
            eps = torch.randn(x.shape[0], latent, generator=g, dtype=torch.float64) if variational else None
            keep = (torch.rand(x.shape, generator=g) >= dropout)
            loss = forward(p, x, variational, eps, keep, dropout, beta)[0]
            opt.zero_grad()
            loss.backward()
            opt.step()
            step += 1
    with torch.no_grad():
        return forward(p, x_all, variational)[3].numpy()
