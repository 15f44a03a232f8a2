"""References for NeuMF (neumf.py, csrc/neumf.hip); helpers only, no tests.

The model, dtype-generic in torch: run in float64 it is the truth, run in float32 on the CPU it is the yardstick of the whole-model tests
(FACTOR times its error is allowed, the project's convention, tests/simplex_ref.py).

    a_u = W1u pm_u + b1      b_i = W1i qm_i      z1 = relu(a_u + b_i)      z_l = relu(W_l z_{l-1} + b_l)
    y(u, i) = <w_g, pg_u * qg_i> + <w_h, z_L> + c

The kernel's scores ('sbr_neumf_score_all', 'sbr_neumf_score_pairs') get a running error bound, computed in float64 next to the truth from
the float32 operands A = a, Bt = b. With u = 2^-24 and gamma(n) = 1.01 n u (the 1.01 covers the second-order terms):

    e_1 = 2 u (|a| + |b|)                     one rounded add, then the ReLU, which is 1-Lipschitz: no condition on the active set
    e_l = |W_l| e_{l-1} + gamma(H_{l-1} + 1) (|W_l| |z_{l-1}| + |b_l|)          a chain of H_{l-1} fmaf from the bias, then the ReLU
    e_m = |w_h| e_L + gamma(H_L + 1) |w_h| |z_L|                                 the same rule, from +0
    e_s = e_m + u (|m + c| + e_m)                                                 the add of c
    e_o = e_s + u (|base + s| + e_s)                                              with accumulate: the add onto the GMF term

The bound holds for any summation order (the kernel's chains run to the next multiple of 4 over +0 cells, which add nothing). It is
derived, not tuned.
"""
import numpy as np
import torch

U = 2.0 ** -24
FACTOR = 8.0
TAILS = ((1,), (3, 2), (5,), (32, 16, 8), (64, 64, 64, 64))
BUS = (1, 63, 65)
IS = (1, 63, 64, 65, 130)


def gamma(n):
    return 1.01 * n * U


# ---- the kernel's operands ------------------------------------------------------------------------------------------------------------------
def kernel_case(Bu, I, widths, seed=0, dead=False):
    """float32 operands of one score call -> dict(A [Bu, H1], Bt [I, H1], Ws, bs (the tail layers), w_h, c, base [Bu, I], widths).
    ``dead``: A is moved down by 64 and the tail biases are <= 0, so that every ReLU of every pair is dead."""
    rng = np.random.default_rng(9000 + 131 * Bu + 17 * I + sum(widths) + 7 * len(widths) + seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    h1 = widths[0]
    c = {'A': f(Bu, h1), 'Bt': f(I, h1), 'widths': tuple(widths),
         'Ws': [(f(widths[l], widths[l - 1]) / np.float32(np.sqrt(widths[l - 1]))).astype(np.float32) for l in range(1, len(widths))],
         'bs': [np.float32(0.25) * f(widths[l]) for l in range(1, len(widths))],
         'w_h': f(widths[-1]), 'c': np.float32(0.375) + np.float32(0.0625) * f(1), 'base': f(Bu, I)}
    if dead:
        c['A'] = (c['A'] - np.float32(64.)).astype(np.float32)
        c['bs'] = [-np.abs(b) for b in c['bs']]
    return c


def pack_tail(c):
    """the packed buffer of the entry: W_2 .. W_L, b_2 .. b_L, w_h, c"""
    return np.concatenate([w.reshape(-1) for w in c['Ws']] + [b.reshape(-1) for b in c['bs']] + [c['w_h'].reshape(-1), c['c'].reshape(-1)]
                          ).astype(np.float32)


def mlp_scores(c, dtype, accumulate):
    """the score of every pair by the torch composition in ``dtype`` on the CPU -> [Bu, I]"""
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dtype)
    z = torch.relu(t(c['A'])[:, None, :] + t(c['Bt'])[None, :, :])
    for W, b in zip(c['Ws'], c['bs']):
        z = torch.relu(z @ t(W).t() + t(b))
    s = z @ t(c['w_h']) + t(c['c'])
    return t(c['base']) + s if accumulate else s


def truth_and_bound(c, accumulate):
    """(float64 scores [Bu, I], the bound on the kernel's error [Bu, I]) as derived in the module docstring"""
    d = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    a, b = d(c['A'])[:, None, :], d(c['Bt'])[None, :, :]
    z = torch.relu(a + b)
    e = 2 * U * (a.abs() + b.abs())
    for W, bias in zip(c['Ws'], c['bs']):
        W, bias = d(W), d(bias)
        n = W.shape[1]
        e = e @ W.abs().t() + gamma(n + 1) * (z.abs() @ W.abs().t() + bias.abs())
        z = torch.relu(z @ W.t() + bias)
    w = d(c['w_h'])
    m = z @ w
    e = e @ w.abs() + gamma(w.shape[0] + 1) * (z.abs() @ w.abs())
    s = m + d(c['c'])
    e = e + U * (s.abs() + e)
    if accumulate:
        s = d(c['base']) + s
        e = e + U * (s.abs() + e)
    return s, e


# ---- the whole model ---------------------------------------------------------------------------------------------------------------------
N_USERS, N_ITEMS = 40, 30
CONFIGS = {'full': dict(gmf_dim=4, mlp_dim=6, mlp_layers=(8, 5, 3)), 'gmf': dict(gmf_dim=4, mlp_dim=0, mlp_layers=()),
           'mlp': dict(gmf_dim=0, mlp_dim=6, mlp_layers=(8, 5, 3))}


def state_keys(gmf_dim, mlp_dim, mlp_layers):
    keys = []
    if gmf_dim:
        keys += ['gmf_user.weight', 'gmf_item.weight']
    if mlp_layers:
        keys += ['mlp_user.weight', 'mlp_item.weight', 'mlp_in_user.weight', 'mlp_in_item.weight', 'mlp_in_bias']
        for l in range(len(mlp_layers) - 1):
            keys += [f'mlp_tail.{l}.weight', f'mlp_tail.{l}.bias']
    if gmf_dim:
        keys.append('out_gmf')
    if mlp_layers:
        keys.append('out_mlp')
    return keys + ['out_bias']


def params(gmf_dim, mlp_dim, mlp_layers, seed=0, n_users=N_USERS, n_items=N_ITEMS, scale=0.5):
    """a float32 state_dict (numpy arrays) with weights large enough that every branch matters"""
    rng = np.random.default_rng(7000 + seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    p = {}
    if gmf_dim:
        p['gmf_user.weight'], p['gmf_item.weight'] = scale * f(n_users, gmf_dim), scale * f(n_items, gmf_dim)
    if mlp_layers:
        h1 = mlp_layers[0]
        p['mlp_user.weight'], p['mlp_item.weight'] = scale * f(n_users, mlp_dim), scale * f(n_items, mlp_dim)
        p['mlp_in_user.weight'] = (f(h1, mlp_dim) / np.sqrt(mlp_dim)).astype(np.float32)
        p['mlp_in_item.weight'] = (f(h1, mlp_dim) / np.sqrt(mlp_dim)).astype(np.float32)
        p['mlp_in_bias'] = np.float32(0.1) * f(h1)
        for l in range(1, len(mlp_layers)):
            p[f'mlp_tail.{l - 1}.weight'] = (f(mlp_layers[l], mlp_layers[l - 1]) / np.sqrt(mlp_layers[l - 1])).astype(np.float32)
            p[f'mlp_tail.{l - 1}.bias'] = np.float32(0.1) * f(mlp_layers[l])
    if gmf_dim:
        p['out_gmf'] = f(gmf_dim)
    if mlp_layers:
        p['out_mlp'] = f(mlp_layers[-1])
    p['out_bias'] = np.float32(0.1) * f(1)
    assert list(p) == state_keys(gmf_dim, mlp_dim, mlp_layers)
    return p


def leaves(p, dtype):
    return {k: torch.from_numpy(v.astype(np.float64)).to(dtype).requires_grad_(True) for k, v in p.items()}


def sides(P, u, i):
    """(a [.., H1] or None, b, gmf user rows times w_g or None, gmf item rows) of the torch leaves ``P``"""
    a = b = gu = gi = None
    if 'mlp_user.weight' in P:
        a = P['mlp_user.weight'][u] @ P['mlp_in_user.weight'].t() + P['mlp_in_bias']
        b = P['mlp_item.weight'][i] @ P['mlp_in_item.weight'].t()
    if 'gmf_user.weight' in P:
        gu, gi = P['gmf_user.weight'][u] * P['out_gmf'], P['gmf_item.weight'][i]
    return a, b, gu, gi


def logits(P, u, i):
    """y of the pairs (u [B], i [B, S]) -> [B, S]; with i [I] every user against every listed item -> [B, I]"""
    u, i = torch.as_tensor(np.asarray(u), dtype=torch.int64), torch.as_tensor(np.asarray(i), dtype=torch.int64)
    a, b, gu, gi = sides(P, u, i)
    if i.dim() == 1:
        b, gi = (None if b is None else b[None]), (None if gi is None else gi[None])
    y = P['out_bias']
    if gu is not None:
        y = y + (gu[:, None, :] * gi).sum(-1)
    if a is not None:
        z = torch.relu(a[:, None, :] + b)
        l = 0
        while f'mlp_tail.{l}.weight' in P:
            z = torch.relu(z @ P[f'mlp_tail.{l}.weight'].t() + P[f'mlp_tail.{l}.bias'])
            l += 1
        y = y + z @ P['out_mlp']
    return y


def model_bound(p, u, i):
    """(float64 logits, the kernel bound on them) for evaluation scores: a and b rounded as the float32 GEMMs leave them is not modelled
    separately; their error, gamma(Dm + 2) (|W1| |pm| + |b1|), enters e_1, and the GMF term's gamma(Dg + 1) |gu| |gi| is added"""
    P = {k: torch.from_numpy(v.astype(np.float64)) for k, v in p.items()}
    u, i = torch.as_tensor(np.asarray(u), dtype=torch.int64), torch.as_tensor(np.asarray(i), dtype=torch.int64)
    y = logits(P, u, i)
    a, b, gu, gi = sides(P, u, i)
    if i.dim() == 1:
        b, gi = (None if b is None else b[None]), (None if gi is None else gi[None])
    e = torch.zeros_like(y)
    s = torch.zeros_like(y)
    if a is not None:
        dm = P['mlp_user.weight'].shape[1]
        ea = gamma(dm + 2) * (P['mlp_user.weight'][u].abs() @ P['mlp_in_user.weight'].abs().t() + P['mlp_in_bias'].abs())
        eb = gamma(dm + 2) * (P['mlp_item.weight'][i].abs() @ P['mlp_in_item.weight'].abs().t())
        if i.dim() == 1:
            eb = eb[None]
        z = torch.relu(a[:, None, :] + b)
        ez = ea[:, None, :] + eb + 2 * U * (a[:, None, :].abs() + b.abs())
        l = 0
        while f'mlp_tail.{l}.weight' in P:
            W, bias = P[f'mlp_tail.{l}.weight'], P[f'mlp_tail.{l}.bias']
            ez = ez @ W.abs().t() + gamma(W.shape[1] + 1) * (z.abs() @ W.abs().t() + bias.abs())
            z = torch.relu(z @ W.t() + bias)
            l += 1
        w = P['out_mlp']
        s = z @ w + P['out_bias']
        e = ez @ w.abs() + gamma(w.shape[0] + 1) * (z.abs() @ w.abs())
        e = e + U * (s.abs() + e)
    else:
        s = s + P['out_bias']
    if gu is not None:
        g = (gu[:, None, :] * gi).sum(-1)
        eg = gamma(gu.shape[-1] + 2) * (gu[:, None, :].abs() * gi.abs()).sum(-1)          # the scaled user row is rounded once more
        e = e + eg + U * (y.abs() + e + eg)
    return y, e


def bce(y, labels):
    return torch.nn.functional.binary_cross_entropy_with_logits(y.flatten(), labels.to(y.dtype).flatten())


def batch(B=24, N=5, seed=0):
    """(u [B], i [B, 1 + N], labels [B, 1 + N] float64 with the positive in column 0)"""
    rng = np.random.default_rng(5000 + seed)
    u = rng.integers(0, N_USERS, B).astype(np.int64)
    i = rng.integers(0, N_ITEMS, (B, 1 + N)).astype(np.int64)
    labels = torch.zeros(B, 1 + N, dtype=torch.float64)
    labels[:, 0] = 1.
    return u, i, labels


def model_grads(p, u, i, labels, dtype):
    """(loss, logits, {parameter: gradient}) by torch autograd in ``dtype`` on the CPU"""
    P = leaves(p, dtype)
    y = logits(P, u, i)
    L = bce(y, labels)
    L.backward()
    return float(L.detach()), y.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in P.items()}


# ---- the evaluation world ------------------------------------------------------------------------------------------------------------------
EVAL_SEED = 0
EVAL_K = 10


def eval_truth(S, seed=EVAL_SEED):
    """The 40 x 30 evaluation world: (dataset, its evaluation view, float32 parameters of the full model, float64 scores [40, 30] with the
    training items at -inf, the kernel bound on them). ``S``: the package."""
    ds = S.SyntheticDataset(N_USERS, N_ITEMS, 300, seed=11, n_negative_samples=3, holdout_per_user=1)
    view = ds.eval_view()
    p = params(seed=100 + seed, scale=1.0, **CONFIGS['full'])
    y, e = model_bound(p, np.arange(N_USERS), np.arange(N_ITEMS))
    excluded = torch.from_numpy(view.exclude_data.toarray() != 0)
    return ds, view, p, y.masked_fill(excluded, -float('inf')), e


def left_out_users(y, e, k=EVAL_K):
    """the users whose float64 top-k list a computation within the bound could change: the k-th and (k + 1)-th scores, or two neighbours
    within the top k, closer than twice the bound (the larger of the two bounds)"""
    val, idx = torch.sort(y, dim=1, descending=True, stable=True)
    eb = torch.gather(e, 1, idx)
    gap = val[:, :k] - val[:, 1:k + 1]
    need = 2 * torch.maximum(eb[:, :k], eb[:, 1:k + 1])
    bad = ~(gap > need)                                           # -inf against -inf counts as too close as well
    return [int(r) for r in torch.nonzero(bad.any(dim=1)).flatten()], idx[:, :k]
