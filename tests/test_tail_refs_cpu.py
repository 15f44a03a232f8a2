"""CPU: the float64 references and bound helpers of tests/test_hip_tail.py, checked without a GPU so that a wrong reference cannot
pass as a kernel bug or hide one: against torch's own batch_norm / autograd in float64, against the oracle's losses evaluated in
float64, and (bounds) against a plain fp32 torch-CPU evaluation of the same formulas, which must lie inside them. The last test
reproduces in numpy the arithmetic of the vectorised BatchNorm statistics before and after they were moved to double: why the
conditioning sweep of the GPU file exists."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_hip_tail as T
from oracle import losses_ref, model_ref

U32 = T.U32
ACT_TORCH = {0: lambda t: t, 1: torch.relu, 2: torch.tanh, 3: torch.sigmoid, 4: F.selu}


def _close(a, b, tol=1e-10):
    assert float((a - b).abs().max()) <= tol * (1 + float(b.abs().max())), float((a - b).abs().max())


@pytest.mark.parametrize('act', [0, 1, 2, 3, 4])
@pytest.mark.parametrize('n,D', [(1, 5), (2, 3), (37, 12), (300, 130)])
def test_batchnorm_references_against_torch_float64(n, D, act):
    x, w, b = T.bn_input(n, D, 3 * n + D, act)
    x, w, b = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    rm, rv = torch.zeros(D, dtype=torch.float64), torch.ones(D, dtype=torch.float64)
    if n > 1:
        y_t = ACT_TORCH[act](F.batch_norm(x, rm, rv, w, b, True, T.MOM32, T.EPS32))
    else:                                                     # torch refuses one row in training mode: the definition by hand
        y_t = ACT_TORCH[act]((x - x.mean(0)) / torch.sqrt(x.var(0, unbiased=False) + T.EPS32) * w + b)
    m, var, rstd = T.ref_bn_stats(x.detach())
    y, pre, _ = T.ref_bn_fwd(x.detach(), w.detach(), b.detach(), m, rstd, act)
    _close(y, y_t.detach(), 1e-7 if act == 4 else 1e-12)      # selu: the kernels' constants are the fp32 roundings of torch's
    if n > 1:
        _close(rm, T.MOM32 * m)
        _close(rv, (1 - T.MOM32) + T.MOM32 * var * n / (n - 1))
    dy = T._rand(n, D, seed=4).double()
    (y_t * dy).sum().backward()
    dx, dw, db = T.ref_bn_bwd(dy, y, x.detach(), w.detach(), m, rstd, act)
    tol = 1e-6 if act == 4 else 1e-9
    _close(dx, x.grad, tol)
    _close(dw, w.grad, tol)
    _close(db, b.grad, tol)
    # relu / selu: nothing is excluded at the kink (see the GPU file's header), so there is no cap to assert; this only checks, for
    # these four shapes, that bn_input puts pre-activations on both sides of 0
    if act in (1, 4) and n > 1:
        assert bool((pre > 0).any()) and bool((pre < 0).any()) and not bool((pre == 0).any())


@pytest.mark.parametrize('n,D,act', [(300, 128, a) for a in range(5)] + [(4097, 12, 2), (70, 3, 4)])
def test_batchnorm_bounds_hold_for_an_fp32_evaluation(n, D, act):
    x, w, b = T.bn_input(n, D, 11 * n + D, act)
    xd = x.double()
    m, var, rstd = T.ref_bn_stats(xd)
    dm, dvar = T.bn_stats_err(xd, n)
    em, er = dm + U32 * m.abs(), 0.5 * dvar / (var + T.EPS32) + U32
    yref, yb = T.bn_fwd_bound(xd, w.double(), b.double(), m, rstd, act, em, er)
    m32, r32 = m.float(), rstd.float()
    sel = (lambda t: T.SELU_SF * torch.where(t > 0, t, T.SELU_AF * (torch.exp(t) - 1)))
    y32 = {0: lambda t: t, 1: torch.relu, 2: torch.tanh, 3: lambda t: 1 / (1 + torch.exp(-t)), 4: sel}[act]((x - m32) * r32 * w + b)
    assert bool(((y32.double() - yref).abs() <= yb).all())
    dy = T._rand(n, D, seed=2)
    yin = yref.float()
    dxr, dwr, dbr = T.ref_bn_bwd(dy.double(), yin.double(), xd, w.double(), m32.double(), r32.double(), act)
    bx, bw, bb = T.bn_bwd_bound(dy.double(), yin.double(), xd, w.double(), m32.double(), r32.double(), act)
    g32 = T.ref_act_grad_from_out(yin.double(), act).float() if act in (0, 1) else \
        {2: 1 - yin * yin, 3: yin * (1 - yin), 4: torch.where(yin > 0, torch.tensor(np.float32(T.SELU_S)), yin + np.float32(T.SELU_SF * T.SELU_AF))}[act]
    dz = dy * g32
    xh = (x - m32) * r32
    s1, s2 = dz.double().sum(0), (dz * xh).double().sum(0)
    dx32 = w * r32 * (dz - (s1 / n).float() - xh * (s2 / n).float())
    assert bool(((dx32.double() - dxr).abs() <= bx).all())
    assert bool(((s2 - dwr).abs() <= bw).all()) and bool(((s1 - dbr).abs() <= bb).all())
    assert bool((bx < 1e-3 * (1 + dxr.abs())).all()), 'a bound that wide would not notice a wrong kernel'


@pytest.mark.parametrize('B,N,D', [(1, 1, 4), (5, 3, 8), (9, 11, 64), (4, 17, 128)])
def test_fused_tail_references_against_autograd(B, N, D):
    z, u, mean, rstd, w, beta = [t.double() for t in T.tail_input(B, N, D, B + D)]
    zr, ur = z.clone().requires_grad_(True), u.clone().requires_grad_(True)
    # the whole tail from its definition: BatchNorm of the R = B N rows with batch statistics, then the scorer
    m = zr.mean(0)
    var = zr.var(0, unbiased=False)
    rs = 1 / torch.sqrt(var + T.EPS32)
    y = ((zr - m) * rs * w + beta).view(B, N, D)
    logits = torch.einsum('bd,bnd->bn', ur, y)
    lg, _, _ = T.ref_score(z, u, m.detach(), rs.detach(), w, beta, N)
    _close(lg, logits.detach())
    g = T._rand(B, N, seed=3).double()
    (logits * g).sum().backward()
    du, s1, s2 = T.ref_pass_a(g, u, z, m.detach(), rs.detach(), w, beta)
    _close(du, ur.grad)
    dx = T.ref_pass_b(g, u, z, m.detach(), rs.detach(), w, torch.cat([s1, s2]))
    _close(dx, zr.grad, 1e-9)
    # fp32 evaluation inside the bounds
    f = [t.float() for t in (z, u, m.detach(), rs.detach(), w, beta)]
    d = [t.double() for t in f]
    lg32 = torch.einsum('bd,bnd->bn', f[1], (((f[0] - f[2]) * f[3]) * f[4] + f[5]).view(B, N, D))
    assert bool(((lg32.double() - T.ref_score(*d, N)[0]).abs() <= T.score_bound(*d, N)).all())
    assert bool((T.score_bound(*d, N) <= 1e-3 * (1 + T.ref_score(*d, N)[0].abs())).all())


@pytest.mark.parametrize('kind,name', [(0, 'bce'), (1, 'bpr'), (2, 'sampled_softmax')])
@pytest.mark.parametrize('B,N', [(1, 1), (3, 2), (300, 11), (64, 16)])
@pytest.mark.parametrize('agg', ['mean', 'sum'])
def test_loss_references_against_the_oracle_in_float64(kind, name, B, N, agg):
    # odd multiples of 1/16 + column / 1024: the fp32 difference of BPR is exact (float64 == the oracle) and neither a logit nor a
    # difference is 0, where the oracle's autograd takes a subgradient of clamp / abs instead of sigmoid(0) - y
    x = (torch.floor(T.loss_logits(B, N, 7 + N) * 8) + 0.5) / 8 + torch.arange(N) / 1024
    lab = torch.zeros(B, N, dtype=torch.float64)
    lab[:, 0] = 1
    if kind == 0:
        lab = torch.rand(B, N, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    cnt = {0: B * N, 1: B * (N - 1), 2: B}[kind]
    if cnt == 0 and agg == 'mean':
        return                                                # mean over no terms: not defined by the oracle either
    scale = 1.0 / cnt if agg == 'mean' else 1.0
    for strat in (('uniform', 'uniform_recbole') if kind == 2 else ('uniform_recbole',)):
        shift = math.log(5000 / max(N - 1, 1)) if (kind == 2 and strat == 'uniform') else 0.0
        xr = x.double().requires_grad_(True)
        ref = losses_ref.RefRecLoss(name, n_items=5000, aggregator=agg, train_neg_strategy=strat, neg_train=max(N - 1, 1)).compute_loss(xr, lab)
        loss, dl = T.ref_rec_loss(kind, x.double(), lab, scale, shift)
        if cnt == 0:
            assert float(loss) == 0.0 and float(dl.abs().max()) == 0.0
            continue
        ref.backward()
        _close(loss, ref.detach(), 1e-12)
        _close(dl, xr.grad, 1e-12)
        bl, bdl = T.rec_loss_bounds(kind, x.double(), lab, scale, shift)
        assert math.isfinite(float(bl)) and bool(torch.isfinite(bdl).all()) and float(bl) <= 1e-4 * (1 + abs(float(loss)))
        if kind == 2:                                         # fp32 evaluation of the chain inside the bound
            xs = x.clone()
            xs[:, 1:] += np.float32(shift)
            lse32 = torch.logsumexp(xs, 1)
            l32, b32 = T.ref_rec_loss(kind, x.double(), lab, scale, float(np.float32(shift))), T.rec_loss_bounds(kind, x.double(), lab, scale, float(np.float32(shift)))
            assert abs(float(scale * (lse32 - x[:, 0]).double().sum()) - float(l32[0])) <= float(b32[0])
            p32 = torch.exp(xs - lse32[:, None])
            p32[:, 0] -= 1
            assert bool((((scale * p32.double()).float().double() - l32[1]).abs() <= b32[1]).all())


@pytest.mark.parametrize('G,N,D,tau', [(1, 1, 3, 1.0), (7, 11, 16, 0.3), (2, 40, 30, 0.05), (1, 177, 8, 0.3)])
def test_infonce_reference_against_the_oracle_in_float64(G, N, D, tau):
    a, b = T._rand(G, N, D, seed=1).double() * 0.5, T._rand(G, N, D, seed=2).double() * 0.5
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = model_ref.info_nce(ar, br, tau)
    ref.backward()
    loss, da, db, _, _ = T.ref_infonce(a, b, tau, 1.0 / (G * N))
    _close(loss, ref.detach(), 1e-12)
    _close(da, ar.grad, 1e-12)
    _close(db, br.grad, 1e-12)
    bl, bA, bB = T.infonce_bounds(a.float().double(), b.float().double(), tau, 1.0 / (G * N))
    l32 = model_ref.info_nce(a.float(), b.float(), tau)
    l64 = T.ref_infonce(a.float().double(), b.float().double(), tau, 1.0 / (G * N))[0]
    assert abs(float(l32) - float(l64)) <= float(bl) and float(bl) <= 1e-3 * (1 + abs(float(l64)))
    assert bool(torch.isfinite(bA).all()) and bool(torch.isfinite(bB).all())


def test_emulated_statistics_arithmetic_before_and_after_the_fix():
    """The table of DESIGN.md ("numerical contract of the BatchNorm statistics"), emulated: with fp32 squares and fp32 per-thread sums
    the cancellation in ss / n - m^2 costs (mean / std)^2 — the variance is off by ~5e-4 at kappa = 256 and misses the rule
    e_k <= 8 max(e_ref, u) from kappa = 32 on —, with double squares and sums it meets the rule at every kappa."""
    n, D = 4096, 8
    for kappa in (0, 1, 8, 32, 256):
        x = T.cond_input(n, D, kappa, 9 + kappa)
        e_ref = T.var_rel_err(T.torch_fp32_bn_var(x), x)
        lim = 8 * max(e_ref, U32)
        e_old = T.var_rel_err(T.emulate_col_reduce_var(x, True), x)
        e_new = T.var_rel_err(T.emulate_col_reduce_var(x, False), x)
        print(f'kappa {kappa}: e_ref {e_ref:.2e}  fp32 squares {e_old:.2e}  double {e_new:.2e}')
        assert e_new <= lim
        if kappa >= 32:
            assert e_old > lim
        if kappa == 256:
            assert e_old > 1e-4
