"""GPU: the back half of the training step — csrc/batchnorm.hip, csrc/fused_tail.hip, csrc/loss.hip — each C entry point against a
plain float64 torch-CPU reference written here from the operation's definition, on both sides of its dispatch conditions.

Conventions: those of tests/test_hip_rowops.py (u = 2^-24; an fp32 sum of m terms in any order errs by at most m u sum|terms|; a
double result rounded once to fp32 errs by at most u |value|, i.e. half an ulp; operands are views inside NaN-filled buffers and
nothing outside the addressed rows may be written). In addition:
  * A reference takes exactly the kernel's INPUTS (fp32 values, widened to float64) and evaluates the definition in float64. Where a
    backward kernel receives the forward's output Y, save_mean and save_rstd as inputs, the reference uses the same given values:
    act'(Y) then has no ambiguity at the kink of relu / selu (the kernel and the reference both ask "Y > 0" of the same number), and
    relu / selu forwards are Lipschitz, so NO element is left out of any comparison in this file (the 0.1 % allowance is not used).
    tests/test_tail_refs_cpu.py checks these references against autograd in float64.
  * Transcendentals: the device's expf / logf / tanhf are specified to 1 - 2 ulp; the bounds allow EXP_ULP = 4 u relative (2 ulp) for
    each call — the one constant here that is not a plain rounding count.
  * Double sums (atomics in arrival order, block partial sums) are compared at 1e-12 relative to sum|terms|: n 2^-53 stays below
    that for every n used here (n <= 4.8e6: 5.3e-10 would be the worst case of a purely sequential sum, but every kernel sums at most
    a few thousand terms per thread before a tree; 1e-12 is asserted because the issue asks for it, and holds)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from hip_testutil import (DEV, EXP_ULP, LIP, NAN, SELU_A, SELU_AF, SELU_S, SELU_SF, U32, S, _L, _assert_bits, _assert_bound, _Buf, _p, _rand, act_grad_err, call,
                          ref_act, ref_act_grad_from_out, stream)

pytestmark = pytest.mark.gpu
U64 = 2.0 ** -53
EPS, MOM = 1e-5, 0.1
EPS32, MOM32 = float(np.float32(EPS)), float(np.float32(MOM))


def _dd(t):
    return t.double()


def _f64dev(t):
    return t.to(torch.float64).to(DEV)


def _zeros64(n):
    return torch.zeros(n, device=DEV, dtype=torch.float64)


@pytest.fixture(params=[False, True], ids=['default', 'deterministic'])
def det(request):
    """runs a test in the default mode and under ops.set_deterministic(True); in the latter no arrival-order launch may be counted.
    The switch is restored whatever happens."""
    ops, L = S().ops, _L().lib()
    prev = ops.set_deterministic(request.param)
    L.sbr_reset_nondeterministic_launches()
    try:
        yield request.param
        if request.param:
            assert int(L.sbr_nondeterministic_launches()) == 0, 'an arrival-order launch ran in deterministic mode'
    finally:
        ops.set_deterministic(prev)


def _same_bits(det, seen, what):
    """deterministic mode: the tensors of two calls agree in every bit"""
    if det and len(seen) == 2:
        for p, q in zip(*seen):
            _assert_bits(p, q, what + ': two deterministic calls')


def _err(fn, *args):
    """the message of the SBR_ERR_ARG an entry point answers with"""
    with pytest.raises(_L().SibrarHipError) as e:
        call(fn, *args)
    return str(e.value)


# =================================================================================================================================
# float64 references and bounds (imported by tests/test_tail_refs_cpu.py)
# =================================================================================================================================
def ref_bn_stats(x, eps=EPS32):
    """x float64 [n, D] -> mean, biased var, rstd (float64)"""
    m = x.mean(0)
    var = ((x - m) ** 2).mean(0)
    return m, var, 1 / torch.sqrt(var + eps)


def bn_stats_err(x, n):
    """bounds of the kernels' double statistics BEFORE the cast to fp32: every sum is a double sum of n terms (error n 2^-53
    sum|terms|), var = ss / n - m m inherits both -> (dm, dvar)"""
    ax = x.abs().mean(0)
    dm = n * U64 * ax
    dvar = n * U64 * (x * x).mean(0) + 2 * x.mean(0).abs() * dm + 4 * U64 * (x * x).mean(0)
    return dm, dvar


def ref_bn_fwd(x, w, b, mean, rstd, act):
    xhat = (x - mean) * rstd
    pre = xhat * w + b
    return ref_act(pre, act), pre, xhat


def bn_fwd_bound(x, w, b, mean, rstd, act, em, er):
    """|Y - ref| for Y = act((X - mean) * rstd * w + b) in fp32 with a mean off by em (absolute) and an rstd off by er (relative):
    subtraction, two multiplications and the addition round once each (a contraction only removes roundings): 4 u on |xhat w| covers
    the three roundings in front of the addition to first order with one to spare for the second-order terms; + u |pre| for the
    addition; the mean's error is scaled by rstd |w|. Then the activation: Lipschitz constant times that, + its own evaluation error
    (tanh: one tanhf; sigmoid: expf, an addition and a division; selu: expf, a subtraction, two multiplications)."""
    y, pre, xhat = ref_bn_fwd(x, w, b, mean, rstd, act)
    bp = (xhat * w).abs() * (4 * U32 + er) + em * (rstd * w).abs() + U32 * pre.abs()
    own = {0: 0.0, 1: 0.0, 2: EXP_ULP * y.abs(), 3: (EXP_ULP + 2 * U32) * y.abs(),
           4: torch.where(pre > 0, U32 * y.abs(), SELU_SF * SELU_AF * (EXP_ULP * torch.exp(pre.clamp_max(0)) + 3 * U32 * torch.expm1(pre.clamp_max(0)).abs()))}[act]
    return y, LIP[act] * bp + own


def ref_bn_bwd(dy, y, x, w, mean, rstd, act):
    """the definition on the kernel's inputs (float64): dz = dY act'(Y); dB = sum dz; dW = sum dz xhat;
    dX = w rstd (dz - mean(dz) - xhat mean(dz xhat))"""
    n = x.shape[0]
    dz = dy * ref_act_grad_from_out(y, act)
    xhat = (x - mean) * rstd
    s1, s2 = dz.sum(0), (dz * xhat).sum(0)
    dx = w * rstd * (dz - s1 / n - xhat * (s2 / n))
    return dx, s2, s1


def colred_terms_per_thread(n, D, blocks=None):
    """how many rows one thread of sbr_col_reduce adds in fp32 before the double tree (RL row lanes, `blocks` row ranges)"""
    RL = 256 // (D // 4) if D % 4 == 0 and 4 <= D <= 1024 else 4
    if blocks is None:
        blocks = max(1, min(512, -(-n // (8 * RL))))
    chunk = -(-n // blocks)
    return -(-chunk // RL)


def bn_bwd_bound(dy, y, x, w, mean, rstd, act):
    """bounds (dX, dW, dB). dz: |dY| e_g + u |dz| (one product). xhat: two roundings. Column sums: the propagated term errors + m u
    sum|terms| for the fp32 accumulation of a thread's m rows (the generic kernel sums in double: the same bound holds with room) +
    u |s| for the final cast. dX: the three terms of the bracket carry their own errors, the two subtractions round relative to at
    most A = |dz| + |mdz| + |xhat mdzx|, w * rstd * (.) rounds twice more."""
    n, D = x.shape
    m = colred_terms_per_thread(n, D)
    g = ref_act_grad_from_out(y, act)
    dz = dy * g
    edz = dy.abs() * act_grad_err(y, act) + U32 * dz.abs()
    xhat = (x - mean) * rstd
    exh = 2 * U32 * xhat.abs()
    s1, s2 = dz.sum(0), (dz * xhat).sum(0)
    e1 = edz.sum(0) + m * U32 * dz.abs().sum(0)
    e2 = (xhat.abs() * edz + dz.abs() * exh + U32 * (dz * xhat).abs()).sum(0) + m * U32 * (dz * xhat).abs().sum(0)
    mdz, mdzx = s1 / n, s2 / n
    emdz, emdzx = e1 / n + U32 * mdz.abs(), e2 / n + U32 * mdzx.abs()
    A = dz.abs() + mdz.abs() + (xhat * mdzx).abs()
    eT = edz + emdz + mdzx.abs() * exh + xhat.abs() * emdzx + U32 * (xhat * mdzx).abs() + 2 * U32 * A
    dx = w * rstd * (dz - mdz - xhat * mdzx)
    return (w * rstd).abs() * eT + 3 * U32 * dx.abs(), e2 + U32 * s2.abs(), e1 + U32 * s1.abs()


# ---- fused tail ------------------------------------------------------------------------------------------------------------------
def ref_score(z, u, mean, rstd, w, beta, N):
    """logits[b, n] = sum_d U[b, d] ((Z[s, d] - mean[d]) rstd[d] w[d] + beta[d]); -> logits [B, N], y [B, N, D], xhat [B, N, D]"""
    B, D = u.shape
    xhat = ((z - mean) * rstd).view(B, N, D)
    y = xhat * w + beta
    return torch.einsum('bd,bnd->bn', u, y), y, xhat


def score_bound(z, u, mean, rstd, w, beta, N):
    """xhat: two roundings; y = fma(xhat, w, beta): one; u * y and the D - 1 additions (fused or not, butterfly or chain): D. All
    relative to |u| (|xhat w| + |beta|) >= |u y| -> (D + 3) u sum_d |u_d| (|xhat_d w_d| + |beta_d|)."""
    B, D = u.shape
    xhat = ((z - mean) * rstd).view(B, N, D)
    return (D + 3) * U32 * torch.einsum('bd,bnd->bn', u.abs(), (xhat * w).abs() + beta.abs())


def ref_pass_a(g, u, z, mean, rstd, w, beta):
    """dU[b] = sum_n G[b, n] y[b, n]; column sums of dy = G[s] U[b] and of dy xhat -> dU [B, D], s1 [D], s2 [D]"""
    B, N = g.shape
    _, y, xhat = ref_score(z, u, mean, rstd, w, beta, N)
    dy = g[:, :, None] * u[:, None, :]
    return torch.einsum('bn,bnd->bd', g, y), dy.sum((0, 1)), (dy * xhat).sum((0, 1))


def pass_a_bound(g, u, z, mean, rstd, w, beta, blocks_users=2):
    """dU: an fma chain of N terms over y (three roundings each): (N + 3) u sum_n |G| (|xhat w| + |beta|). Column sums: dy is one
    product (u), dy * xhat adds xhat's two roundings and the fma; a thread adds the N rows of each of its users in fp32 (m terms),
    then the lanes and blocks are added in double."""
    B, N = g.shape
    D = u.shape[1]
    RL = 256 // (D // 4)
    blocks = max(1, min(512, -(-B // (blocks_users * RL))))
    m = -(-(-(-B // blocks)) // RL) * N
    xhat = ((z - mean) * rstd).view(B, N, D)
    dy = g[:, :, None] * u[:, None, :]
    bdu = (N + 3) * U32 * torch.einsum('bn,bnd->bd', g.abs(), (xhat * w).abs() + beta.abs())
    return bdu, (m + 1) * U32 * dy.abs().sum((0, 1)), (m + 3) * U32 * (dy * xhat).abs().sum((0, 1))


def ref_pass_b(g, u, z, mean, rstd, w, ws):
    """dX[s] = w rstd (G[s] U[b] - ws[0:D] / R - xhat ws[D:2D] / R) on the GIVEN totals ws (float64)"""
    B, N = g.shape
    D = u.shape[1]
    R = B * N
    xhat = ((z - mean) * rstd).view(B, N, D)
    dy = g[:, :, None] * u[:, None, :]
    return (w * rstd * (dy - ws[:D] / R - xhat * (ws[D:] / R))).view(R, D)


def pass_b_bound(g, u, z, mean, rstd, w, ws):
    """the bracket: G u (one rounding), mdz = (float)(ws / R) (one), xhat mdzx (xhat's two, mdzx's cast, the product: four), two
    subtractions relative to at most A -> 6 u A; w * rstd * (.): two more roundings, + one for second order"""
    B, N = g.shape
    D = u.shape[1]
    R = B * N
    xhat = ((z - mean) * rstd).view(B, N, D)
    dy = g[:, :, None] * u[:, None, :]
    A = dy.abs() + (ws[:D] / R).abs() + (xhat * (ws[D:] / R)).abs()
    dx = w * rstd * (dy - ws[:D] / R - xhat * (ws[D:] / R))
    return ((w * rstd).abs() * 6 * U32 * A + 3 * U32 * dx.abs()).view(R, D)


# ---- recommendation losses -------------------------------------------------------------------------------------------------------
def _bce_terms(x, y):
    return torch.clamp(x, min=0) - x * y + torch.log1p(torch.exp(-x.abs()))


def ref_rec_loss(kind, x, labels, scale, shift):
    """x: the fp32 logits widened to float64 [B, N]; labels float64; -> loss (float64 scalar), dlogits [B, N] for upstream gradient 1,
    and the per-element error bound of dlogits given an absolute error ex of the logits (zeros: the logits are the kernel's input).
    BPR follows the reference in taking the difference x0 - xj in fp32."""
    B, N = x.shape
    if kind == 0:
        return scale * _bce_terms(x, labels).sum(), scale * (torch.sigmoid(x) - labels)
    if kind == 1:
        d = (x[:, :1].float() - x[:, 1:].float()).double()
        y = labels[:, :1]
        gd = scale * (torch.sigmoid(d) - y)
        return scale * _bce_terms(d, y).sum(), torch.cat([gd.sum(1, keepdim=True), -gd], 1)
    xs = x.clone()
    xs[:, 1:] += shift
    lse = torch.logsumexp(xs, 1)
    p = torch.exp(xs - lse[:, None])
    p0 = p.clone()
    p0[:, 0] -= 1
    return scale * (lse - x[:, 0]).sum(), scale * p0


def rec_loss_bounds(kind, x, labels, scale, shift, ex=None):
    """-> (absolute bound of the loss, elementwise bound of dlogits). ex: absolute error of the logits the kernel works on (the fused
    scorer + loss kernel computes them itself), None = exact inputs.
    BCE: double arithmetic on (double)x: loss 1e-12 sum|terms|; dlogits = (float)(scale (sigmoid - y)): one rounding; an error ex of
    the logit moves sigmoid by at most ex / 4 and the term by at most ex (|d term / dx| = |sigmoid - y| <= 1).
    BPR: d = x0 - xj in fp32 is what the reference does too (no error with exact inputs; ex_0 + ex_j + u |d| otherwise); the positive
    column is a double sum of the N - 1 gradients, rounded once.
    Sampled softmax (fp32 chain): shifted logits round once (u |x + shift|); every exponent x_j - mx rounds once (u |x_j - mx|) and its
    expf errs by EXP_ULP, both relative to the term, i.e. weighted by the softmax p_j in d lse; the N - 1 additions N u; logf EXP_ULP
    |log se| ; the final addition u |lse|. The gradient's exponent x_j - lse carries ex_j + e_lse + u |x_j - lse|, its expf EXP_ULP; the
    subtraction of 1 and the two conversions round once each."""
    B, N = x.shape
    z = torch.zeros_like(x) if ex is None else ex
    loss, dl = ref_rec_loss(kind, x, labels, scale, shift)
    if kind == 0:
        t = _bce_terms(x, labels)
        return scale * (1e-12 * t.abs().sum() + z.sum()), scale * 0.25 * z + U32 * dl.abs() + 1e-30
    if kind == 1:
        d = (x[:, :1].float() - x[:, 1:].float()).double()
        ed = torch.zeros_like(d) if ex is None else z[:, :1] + z[:, 1:] + U32 * d.abs()
        t = _bce_terms(d, labels[:, :1])
        egd = scale * 0.25 * ed
        bdl = torch.cat([egd.sum(1, keepdim=True), egd], 1) + U32 * dl.abs() + 1e-30
        return scale * (1e-12 * t.abs().sum() + ed.sum()), bdl
    xs = x.clone()
    xs[:, 1:] += shift
    exs = z.clone()
    if shift != 0:
        exs[:, 1:] += U32 * xs[:, 1:].abs()
    mx = xs.max(1, keepdim=True).values
    lse = torch.logsumexp(xs, 1, keepdim=True)
    p = torch.exp(xs - lse)
    se_log = (lse - mx).abs()
    e_lse = (p * (exs + U32 * (xs - mx).abs() + EXP_ULP)).sum(1, keepdim=True) + N * U32 + EXP_ULP * se_log + U32 * lse.abs() + U32 * mx.abs()
    term = lse[:, 0] - x[:, 0]
    bl = scale * ((e_lse[:, 0] + z[:, 0] + U32 * term.abs()).sum() + 1e-12 * term.abs().sum())
    p0 = p.clone()
    p0[:, 0] -= 1
    bdl = scale * (p * (exs + e_lse + U32 * (xs - lse).abs() + EXP_ULP) + 2 * U32 * p0.abs()) + U32 * dl.abs() + 1e-30
    return bl, bdl


# ---- InfoNCE ---------------------------------------------------------------------------------------------------------------------
def ref_infonce(a, b, tau, scale):
    """a, b float64 [G, N, D] -> loss = scale sum_g sum_i (lse_row_i + lse_col_i - 2 L_ii), L = a b^T / tau; dA, dB for upstream 1"""
    L = torch.einsum('gid,gjd->gij', a, b) / tau
    lr, lc = torch.logsumexp(L, 2), torch.logsumexp(L, 1)
    diag = torch.diagonal(L, dim1=1, dim2=2)
    loss = scale * (lr + lc - 2 * diag).sum()
    Gm = (scale / tau) * (torch.exp(L - lr[:, :, None]) + torch.exp(L - lc[:, None, :]) - 2 * torch.eye(L.shape[1], dtype=L.dtype))
    return loss, torch.einsum('gij,gjd->gid', Gm, b), torch.einsum('gji,gjd->gid', Gm, a), L, Gm


def infonce_bounds(a, b, tau, scale):
    """eL: the fp32 dot product of D terms, the rounding of inv_tau = 1 / tau and the scaling by it: (D + 2) roundings, (D + 3) u
    sum|a b| / tau asserted. The GEMM route (sbr_infonce_gemm_*) has the same count and needs no constant of its own: its products are
    fp32 fmaf chains on the matrix cores (D terms), it scales the stored product by inv_tau wherever it reads it (the same rounding
    every time), its log-sum-exps are wave sums of N terms, dA = G B is an N-term chain, and dB = G^T A is N products whose split-K
    slab sums are a different parenthesisation of the same N - 1 additions. A log-sum-exp is 1-Lipschitz in the max norm: e_lse = max eL over the row /
    column + the chain's own roundings (as for sampled softmax). Loss terms lse - L_ii: + eL_ii + u |term|. Gradient matrix
    G_ij = up (p_r + p_c - 2 delta): each p errs relatively by its exponent's error + EXP_ULP; three more roundings; dA = G B: N
    products and additions ((N + 2) u sum|G b|) + the propagated error of G."""
    Gn, N, D = a.shape
    loss, dA, dB, L, Gm = ref_infonce(a, b, tau, scale)
    eL = (D + 3) * U32 * torch.einsum('gid,gjd->gij', a.abs(), b.abs()) / tau
    lr, lc = torch.logsumexp(L, 2), torch.logsumexp(L, 1)

    def own(lse, mxv):
        return N * U32 + EXP_ULP * (1 + (lse - mxv).abs()) + U32 * (lse.abs() + mxv.abs()) + U32 * (L.abs().amax((1, 2))[:, None] + mxv.abs())
    elr = eL.amax(2) + own(lr, L.amax(2))
    elc = eL.amax(1) + own(lc, L.amax(1))
    diag, ediag = torch.diagonal(L, dim1=1, dim2=2), torch.diagonal(eL, dim1=1, dim2=2)
    bl = scale * ((elr + elc + 2 * ediag + U32 * ((lr - diag).abs() + (lc - diag).abs())).sum() + 1e-12 * ((lr - diag).abs() + (lc - diag).abs()).sum())
    pr, pc = torch.exp(L - lr[:, :, None]), torch.exp(L - lc[:, None, :])
    up = scale / tau
    eG = up * (pr * (eL + elr[:, :, None] + U32 * (L - lr[:, :, None]).abs() + EXP_ULP) + pc * (eL + elc[:, None, :] + U32 * (L - lc[:, None, :]).abs() + EXP_ULP)) \
        + 5 * U32 * up * (pr + pc + 2 * torch.eye(N, dtype=L.dtype))
    bA = torch.einsum('gij,gjd->gid', eG, b.abs()) + (N + 2) * U32 * torch.einsum('gij,gjd->gid', Gm.abs(), b.abs())
    bB = torch.einsum('gji,gjd->gid', eG, a.abs()) + (N + 2) * U32 * torch.einsum('gji,gjd->gid', Gm.abs(), a.abs())
    return bl, bA, bB


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def bn_input(n, D, seed, act):
    """fp32 x with column means in [-2, 2] and scales in [0.5, 2.5]: relu / selu pre-activations fall on both sides of 0"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, D, generator=g) * (0.5 + 2 * torch.rand(D, generator=g)) + (4 * torch.rand(D, generator=g) - 2)
    w = torch.rand(D, generator=g) + 0.5
    w[::3] *= -1
    b = torch.randn(D, generator=g) * 0.3
    return x, w, b


def cond_input(n, D, kappa, seed):
    return torch.randn(n, D, generator=torch.Generator().manual_seed(seed)) + float(kappa)


def emulate_col_reduce_var(x, fp32_squares=True):
    """numpy emulation of the arithmetic of the vectorised statistics kernel BEFORE the fix (fp32 x * x, sequential fp32 sums of a
    thread's rows, double across row lanes and blocks) / after it (double from the first addition) -> biased variance per column"""
    x = x.numpy()
    n, D = x.shape
    RL = 256 // (D // 4)
    blocks = max(1, min(512, -(-n // (8 * RL))))
    chunk = -(-n // blocks)
    s, q = np.zeros(D), np.zeros(D)
    for bk in range(blocks):
        lo, hi = bk * chunk, min(n, (bk + 1) * chunk)
        for rl in range(RL):
            rows = x[lo + rl:hi:RL]
            if rows.shape[0] == 0:
                continue
            if fp32_squares:
                sq = rows * rows
                a, c = np.zeros(D, np.float32), np.zeros(D, np.float32)
                for r in range(rows.shape[0]):
                    a += rows[r]
                    c += sq[r]
                s += a.astype(np.float64)
                q += c.astype(np.float64)
            else:
                r64 = rows.astype(np.float64)
                s += r64.sum(0)
                q += (r64 * r64).sum(0)
    m = s / n
    return torch.from_numpy(np.maximum(q / n - m * m, 0.0))


def var_rel_err(var, x):
    v = x.double().var(0, unbiased=False)
    return float(((var.double() - v).abs() / v).max())


def torch_fp32_bn_var(x):
    """biased batch variance of torch CPU fp32 F.batch_norm (training mode), read back through running_var with momentum 1"""
    n, D = x.shape
    rm, rv = torch.zeros(D), torch.ones(D)
    torch.nn.functional.batch_norm(x, rm, rv, None, None, True, 1.0, EPS)
    return rv.double() * ((n - 1) / n if n > 1 else 1.0)


# =================================================================================================================================
# BatchNorm
# =================================================================================================================================
def _rl(D):
    return 256 // (D // 4) if D % 4 == 0 and 4 <= D <= 1024 else 4


def _bn_cases():
    cases = []
    q = 0
    for D in (1, 3, 4, 12, 64, 100, 128, 130, 256, 1000, 1024, 1028):
        RL = _rl(D)
        ns = sorted({1, 2, 4 * RL - 1, 4 * RL, 4 * RL + 1, 8 * RL - 1, 8 * RL, 8 * RL + 1, 16 * RL + 3})
        for n in ns:
            if n >= 1:
                cases.append((n, D, q % 5, 0, 'x'))
                q += 1
    for act in range(5):                                     # every activation on the vectorised and on the generic path
        cases += [(300, 128, act, 0, 'x'), (300, 130, act, 0, 'x')]
    cases += [(70, 128, 1, 1, 'x'), (70, 128, 4, 2, 'x')]     # X 4 / 8 bytes off: forward and backward take the generic kernels
    cases += [(70, 128, 2, 1, w) for w in ('dy', 'y', 'mean', 'rstd')]      # one backward operand off at a time: vec_ok fails
    cases += [(4609, 1024, 1, 0, 'x'),                        # 512-block cap of the vectorised statistics with EMPTY trailing blocks
              #   (chunk 10: blocks 461 .. 511 start past n) and 18,436 > 4,096 blocks of the apply kernels
              (40000, 3, 4, 0, 'x'),                          # 625 > 512 blocks of the generic statistics kernels
              (66000, 64, 3, 0, 'x')]                         # 516 > 512 row ranges at D = 64 (RL = 16), apply capped too (16,500 blocks)
    return cases


@pytest.mark.parametrize('n,D,act,off,which', _bn_cases())
def test_batchnorm_fwd_stats_eval_bwd(n, D, act, off, which, det):
    """sbr_bn_train_fwd, sbr_bn_train_stats, sbr_bn_eval_fwd and sbr_bn_train_bwd on one input. Statistics: save_mean / save_rstd within
    half an fp32 ulp of the float64 value + the double sums' own error; running statistics: the fp32 update (1 - momentum) r + momentum
    v rounds three times; num_batches_tracked + 1; with NULL running statistics and a NULL counter the same save_mean / save_rstd bits.
    Workspace: totals in ws[0 .. 2 D) are not promised by the forward (the finaliser consumes the replicas), all 16 replicas zero after
    every call, a second call on the same workspace inside the same bounds. Backward on the reference's own Y / mean / rstd (rounded to
    fp32) as inputs: dX, dW, dB; totals left in ws[0 .. 2 D) (what sbr_bn_score_bwd_apply reads); replicas zero.
    Deterministic mode (the `det` fixture): the same calls, the same bounds, the two calls of every loop bit-identical, no
    arrival-order launch; where the fixed-slot form does not exist (D % 4 != 0, D > 1024, a misaligned operand) the entry point says
    "no deterministic form" and writes nothing."""
    fwd_ok = D % 4 == 0 and 4 <= D <= 1024 and not (off and which == 'x')
    bwd_ok = fwd_ok and off == 0
    x, w, b = bn_input(n, D, 1000 * D + n, act)
    xd = _dd(x)
    m, var, rstd = ref_bn_stats(xd)
    dm, dvar = bn_stats_err(xd, n)
    em = dm + U32 * m.abs()
    er = 0.5 * dvar / (var + EPS32) + U32
    X = _Buf(n, D, off=off if which == 'x' else 0, data=x)
    Y = _Buf(n, D, off=off if which == 'x' else 0)
    wd_, bd_ = w.to(DEV), b.to(DEV)
    rm0, rv0 = _rand(D, seed=5) * 0.5, _rand(D, seed=6).abs() + 0.5
    rm, rv, nb = rm0.to(DEV), rv0.to(DEV), torch.full((1,), 41, dtype=torch.int64, device=DEV)
    sm_, sr_ = _Buf(1, D), _Buf(1, D)
    ws = _zeros64(34 * D)
    yref, ybound = bn_fwd_bound(xd, _dd(w), _dd(b), m, rstd, act, em, er)
    if det and not fwd_ok:
        assert 'no deterministic form' in _err('sbr_bn_train_fwd', X.ptr, Y.ptr, n, D, _p(wd_), _p(bd_), _p(rm), _p(rv), _p(nb), sm_.ptr, sr_.ptr, _p(ws), EPS, MOM, act, stream())
        assert 'no deterministic form' in _err('sbr_bn_train_stats', X.ptr, n, D, None, None, None, sm_.ptr, sr_.ptr, _p(ws), EPS, MOM, stream())
        for t in (Y, sm_, sr_):
            t.check_untouched([], 'refused')
        assert int(nb) == 41 and bool((ws == 0).all())
    seen = []
    for rep in range(2 if (fwd_ok or not det) else 0):
        call('sbr_bn_train_fwd', X.ptr, Y.ptr, n, D, _p(wd_), _p(bd_), _p(rm), _p(rv), _p(nb), sm_.ptr, sr_.ptr, _p(ws), EPS, MOM, act, stream())
        assert bool((ws[2 * D:] == 0).all()), 'replicas not zeroed'
        got_m, got_r = sm_.check_untouched(None, 'save_mean')[0], sr_.check_untouched(None, 'save_rstd')[0]
        _assert_bound(got_m, m, em, 'save_mean')
        _assert_bound(got_r, rstd, rstd * er, 'save_rstd')
        _assert_bound(Y.check_untouched(None, 'Y'), yref, ybound, f'Y act {act}')
        seen.append((Y.host(), got_m, got_r))
        if rep == 0:
            unb = var * (n / (n - 1)) if n > 1 else var
            ra, rb = (1 - MOM32) * _dd(rm0), MOM32 * m
            _assert_bound(rm.cpu(), ra + rb, 4 * U32 * (ra.abs() + rb.abs()) + MOM32 * dm, 'running_mean')
            va, vb = (1 - MOM32) * _dd(rv0), MOM32 * unb
            _assert_bound(rv.cpu(), va + vb, 4 * U32 * (va.abs() + vb.abs()) + MOM32 * dvar * (n / max(n - 1, 1)), 'running_var')
        assert int(nb) == 42 + rep
    _same_bits(det, seen, 'sbr_bn_train_fwd')
    # statistics alone, NULL running statistics / counter: the same producer, the same bits up to the atomics' order
    if fwd_ok or not det:
        sm2, sr2 = _Buf(1, D), _Buf(1, D)
        call('sbr_bn_train_stats', X.ptr, n, D, None, None, None, sm2.ptr, sr2.ptr, _p(ws), EPS, MOM, stream())
        assert bool((ws[2 * D:] == 0).all())
        _assert_bound(sm2.check_untouched(None, 'save_mean (stats)')[0], m, em, 'save_mean (stats)')
        _assert_bound(sr2.check_untouched(None, 'save_rstd (stats)')[0], rstd, rstd * er, 'save_rstd (stats)')
        if det:                                               # the same fixed-order producer as inside sbr_bn_train_fwd: the same bits
            _assert_bits(sm2.host()[0], seen[0][1], 'sbr_bn_train_stats vs sbr_bn_train_fwd')
            _assert_bits(sr2.host()[0], seen[0][2], 'sbr_bn_train_stats vs sbr_bn_train_fwd')
    # eval mode on given running statistics: (x - rm) / sqrtf(rv + eps) * w + b -> rv + eps, sqrtf, the division: 3 more roundings
    Ye = _Buf(n, D, off=off if which == 'x' else 0)
    call('sbr_bn_eval_fwd', X.ptr, Ye.ptr, n, D, _p(wd_), _p(bd_), _p(rm), _p(rv), EPS, act, stream())
    rme, rve = _dd(rm.cpu()), _dd(rv.cpu())
    re_ = 1 / torch.sqrt(rve + EPS32)
    yre, ybe = bn_fwd_bound(xd, _dd(w), _dd(b), rme, re_, act, torch.zeros(D, dtype=torch.float64), torch.full((D,), 3 * U32, dtype=torch.float64))
    _assert_bound(Ye.check_untouched(None, 'Y eval'), yre, ybe, 'Y eval')
    # backward on given fp32 inputs
    y32, m32, r32 = yref.float(), m.float(), rstd.float()
    dy = _rand(n, D, seed=D + 7)
    o = lambda name: off if which == name else 0
    Xb, dYb, Yb = _Buf(n, D, off=o('x'), data=x), _Buf(n, D, off=o('dy'), data=dy), _Buf(n, D, off=o('y'), data=y32)
    Mb, Rb = _Buf(1, D, off=o('mean'), data=m32[None]), _Buf(1, D, off=o('rstd'), data=r32[None])
    dXb, dWb, dBb = _Buf(n, D, off=o('x')), _Buf(1, D), _Buf(1, D)
    dxr, dwr, dbr = ref_bn_bwd(_dd(dy), _dd(y32), xd, _dd(w), _dd(m32), _dd(r32), act)
    bx, bw, bb = bn_bwd_bound(_dd(dy), _dd(y32), xd, _dd(w), _dd(m32), _dd(r32), act)
    if det and not bwd_ok:
        assert 'no deterministic form' in _err('sbr_bn_train_bwd', dYb.ptr, Yb.ptr, Xb.ptr, dXb.ptr, n, D, _p(wd_), Mb.ptr, Rb.ptr, dWb.ptr, dBb.ptr, _p(ws), act, stream())
        for t in (dXb, dWb, dBb):
            t.check_untouched([], 'refused')
        return
    seen = []
    for rep in range(2):
        call('sbr_bn_train_bwd', dYb.ptr, Yb.ptr, Xb.ptr, dXb.ptr, n, D, _p(wd_), Mb.ptr, Rb.ptr, dWb.ptr, dBb.ptr, _p(ws), act, stream())
        assert bool((ws[2 * D:] == 0).all()), 'replicas not zeroed (backward)'
        _assert_bound(dXb.check_untouched(None, 'dX'), dxr, bx, f'dX act {act}')
        _assert_bound(dWb.check_untouched(None, 'dW')[0], dwr, bw, 'dW')
        _assert_bound(dBb.check_untouched(None, 'dB')[0], dbr, bb, 'dB')
        _assert_bound(ws[:D].cpu(), dbr, bb, 'ws totals (sum dz)')
        _assert_bound(ws[D:2 * D].cpu(), dwr, bw, 'ws totals (sum dz xhat)')
        seen.append((dXb.host(), dWb.host(), dBb.host(), ws[:2 * D].cpu()))
    _same_bits(det, seen, 'sbr_bn_train_bwd')


@pytest.mark.parametrize('D', [4, 128, 130])
def test_batchnorm_constant_column_and_single_row(D):
    """A constant column: var = ss / n - m m may come out a few double ulps below zero; the clamp makes it 0 and rstd = 1 / sqrt(eps)
    (within the double rounding of the cancellation: |var| <= 4 n 2^-53 c^2, relative to eps), Y = b there. n = 1: every column is
    constant, the running variance takes the `n = 1` branch (no n / (n - 1))."""
    for n in (1, 37, 1000):
        x, w, b = bn_input(n, D, 77 + n, 0)
        x[:, 0] = 0.1 + 1e-3                                  # a value whose square is not a double-exact multiple: cancellation noise
        if D > 2:
            x[:, 2] = -3.0
        xd = _dd(x)
        m, var, rstd = ref_bn_stats(xd)
        dm, dvar = bn_stats_err(xd, n)
        X, Y, sm_, sr_ = _Buf(n, D, data=x), _Buf(n, D), _Buf(1, D), _Buf(1, D)
        rm, rv, wd_, bd_ = torch.zeros(D, device=DEV), torch.ones(D, device=DEV), w.to(DEV), b.to(DEV)
        ws = _zeros64(34 * D)
        call('sbr_bn_train_fwd', X.ptr, Y.ptr, n, D, _p(wd_), _p(bd_), _p(rm), _p(rv), None, sm_.ptr, sr_.ptr, _p(ws), EPS, MOM, 0, stream())
        got_r = sr_.host()[0]
        er = 0.5 * dvar / (var + EPS32) + U32
        _assert_bound(got_r, rstd, rstd * er, 'rstd')
        const = [0, 2] if D > 2 else [0]
        if n == 1:
            const = list(range(D))
        for c in const:
            assert float(got_r[c]) <= float(np.float32(1 / math.sqrt(EPS32))) * (1 + 2 * U32), 'the clamp: rstd must not exceed 1 / sqrt(eps)'
        yref, yb = bn_fwd_bound(xd, _dd(w), _dd(b), m, rstd, 0, dm + U32 * m.abs(), er)
        _assert_bound(Y.check_untouched(None, 'Y'), yref, yb, 'Y')
        unb = var * (n / (n - 1)) if n > 1 else var
        vb = MOM32 * unb + (1 - MOM32)
        _assert_bound(rv.cpu(), vb, 4 * U32 * vb.abs() + MOM32 * dvar * (n / max(n - 1, 1)), 'running_var')


def test_bn_finalize_stats_on_hand_written_pending_sums():
    """sbr_bn_finalize_stats: pending sums spread by hand over replicas 1, 2, 7 and 16 (layout [1 + replica][2][D]); mean = s / n,
    var = ss / n - mean^2 (one negative: clamped to 0), running statistics with the unbiased factor n / (n - 1), replicas zeroed."""
    D, n = 6, 10
    s = torch.tensor([10.0, -20.0, 0.0, 5.0, 1e3, 3.0], dtype=torch.float64)
    ss = torch.tensor([30.0, 50.0, 4.0, 2.5 - 1e-9, 1e5 + 7.0, 1.0], dtype=torch.float64)    # column 3: var = -1e-10 -> 0
    ws = torch.zeros(17, 2, D, dtype=torch.float64)
    for r, f in ((1, 0.5), (2, 0.25), (7, 0.125), (16, 0.125)):
        ws[r, 0], ws[r, 1] = s * f, ss * f
    wsd = ws.to(DEV)
    rm0, rv0 = _rand(D, seed=1), _rand(D, seed=2).abs()
    rm, rv, nb = rm0.to(DEV), rv0.to(DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    sm_, sr_ = _Buf(1, D), _Buf(1, D)
    call('sbr_bn_finalize_stats', n, D, _p(rm), _p(rv), _p(nb), sm_.ptr, sr_.ptr, _p(wsd), EPS, MOM, stream())
    m = s / n
    var = (ss / n - m * m).clamp_min(0)
    assert float(var[3]) == 0.0 and float(var[5]) > 0
    rstd = 1 / torch.sqrt(var + EPS32)
    _assert_bound(sm_.check_untouched(None, 'mean')[0], m, U32 * m.abs(), 'mean')
    _assert_bound(sr_.check_untouched(None, 'rstd')[0], rstd, 2 * U32 * rstd, 'rstd')
    unb = var * n / (n - 1)
    ra, rb = (1 - MOM32) * _dd(rm0), MOM32 * m
    _assert_bound(rm.cpu(), ra + rb, 4 * U32 * (ra.abs() + rb.abs()), 'running_mean')
    va, vb = (1 - MOM32) * _dd(rv0), MOM32 * unb
    _assert_bound(rv.cpu(), va + vb, 4 * U32 * (va.abs() + vb.abs()), 'running_var')
    assert int(nb) == 1 and bool((wsd[1:] == 0).all())
    assert 'bad arguments' in _err('sbr_bn_finalize_stats', 0, D, None, None, None, sm_.ptr, sr_.ptr, _p(wsd), EPS, MOM, stream())


def test_batchnorm_refuses_empty_batches_and_null_operands():
    t = torch.zeros(64, device=DEV)
    ws = _zeros64(34 * 4)
    assert 'at least one row' in _err('sbr_bn_train_fwd', _p(t), _p(t), 0, 4, _p(t), _p(t), None, None, None, _p(t), _p(t), _p(ws), EPS, MOM, 0, stream())
    assert 'null operand' in _err('sbr_bn_train_fwd', None, _p(t), 4, 4, _p(t), _p(t), None, None, None, _p(t), _p(t), _p(ws), EPS, MOM, 0, stream())
    assert 'at least one row' in _err('sbr_bn_train_stats', _p(t), 0, 4, None, None, None, _p(t), _p(t), _p(ws), EPS, MOM, stream())
    assert 'empty batch' in _err('sbr_bn_train_bwd', _p(t), _p(t), _p(t), _p(t), 0, 4, _p(t), _p(t), _p(t), _p(t), _p(t), _p(ws), 0, stream())
    call('sbr_bn_eval_fwd', None, None, 0, 4, None, None, None, None, EPS, 0, stream())        # n = 0: nothing to do, no error


# ---- the conditioning sweep ------------------------------------------------------------------------------------------------------
def _variance_from_running(rv, n):
    return rv.double().cpu() * ((n - 1) / n)


@pytest.mark.parametrize('n', [4096, 90112])
@pytest.mark.parametrize('kappa', [0, 1, 8, 32, 256])
def test_variance_conditioning_of_the_three_statistics_producers(kappa, n):
    """x = randn + kappa (mean / std = kappa). On the same fp32 input: e_ref = relative error of the biased batch variance of torch CPU
    fp32 F.batch_norm against float64, e_k the same for each producer (all read back through running_var with momentum 1, so both carry
    the same final fp32 rounding), worst column. Required: e_k <= 8 max(e_ref, u) (8: e_ref is one draw of rounding noise and moves by
    2 - 4 x between columns and kappa). Producers: the generic kernel (X 4 bytes off a 16-byte boundary), the vectorised kernel
    (aligned X), and the statistics epilogue of sbr_gemm_split_bnstats_f32 (N = K = 128, bias = kappa, unit-variance output).
    Before the fix (fp32 squares, fp32 partial sums) 4 of the 10 cases failed: e_k / e_ref of the vectorised kernel / the epilogue was
    7.0 / 8.3 at kappa = 8, 139 / 113 at kappa = 32 and 3,862 / 9,786 at kappa = 256 (n = 4096), 416 / 280 at kappa = 256 (n = 90112);
    the full table is in DESIGN.md section 4.5."""
    D = 8
    x = cond_input(n, D, kappa, 9 + kappa)
    e_ref = var_rel_err(torch_fp32_bn_var(x), x)
    lim = 8 * max(e_ref, U32)
    out = {}
    for name, off in (('generic', 1), ('vectorised', 0)):
        X, sm_, sr_ = _Buf(n, D, off=off, data=x), _Buf(1, D), _Buf(1, D)
        rm, rv = torch.zeros(D, device=DEV), torch.ones(D, device=DEV)
        ws = _zeros64(34 * D)
        call('sbr_bn_train_stats', X.ptr, n, D, _p(rm), _p(rv), None, sm_.ptr, sr_.ptr, _p(ws), EPS, 1.0, stream())
        out[name] = var_rel_err(_variance_from_running(rv, n), x)
    # GEMM epilogue
    N = K = 128
    g = torch.Generator().manual_seed(3 + kappa)
    a, wt = torch.randn(n, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.full((N,), float(kappa))
    ad, wd_, bd_, c = a.to(DEV), wt.to(DEV), bias.to(DEV), torch.empty(n, N, device=DEV)
    ws, arrive = _zeros64(17 * 2 * N), torch.zeros(1, dtype=torch.int64, device=DEV)
    rm, rv = torch.zeros(N, device=DEV), torch.ones(N, device=DEV)
    sm_, sr_ = _Buf(1, N), _Buf(1, N)
    call('sbr_gemm_split_bnstats_f32', _p(ad), K, _p(wd_), K, _p(bd_), _p(c), N, n, N, K, 0, _p(ws), _p(arrive), _p(rm), _p(rv), None,
         sm_.ptr, sr_.ptr, EPS, 1.0, stream())
    ch = c.cpu()
    e_ref_g = var_rel_err(torch_fp32_bn_var(ch), ch)
    out['gemm epilogue'] = var_rel_err(_variance_from_running(rv, n), ch)
    assert bool((ws[2 * N:] == 0).all()) and int(arrive) == 0
    refs = {'generic': e_ref, 'vectorised': e_ref, 'gemm epilogue': e_ref_g}
    print(f'\nconditioning n={n} kappa={kappa}: ' + ' | '.join(f'{k} e_k {v:.2e} e_ref {refs[k]:.2e} ratio {v / max(refs[k], U32):.2f}' for k, v in out.items()))
    assert out['generic'] <= lim, ('generic', out['generic'], e_ref)
    assert out['vectorised'] <= lim, ('vectorised', out['vectorised'], e_ref)
    assert out['gemm epilogue'] <= 8 * max(e_ref_g, U32), ('gemm epilogue', out['gemm epilogue'], e_ref_g)


# =================================================================================================================================
# fused tail
# =================================================================================================================================
TAIL_DS = [4, 8, 16, 32, 64, 128, 256]


def tail_input(B, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B * N, D, generator=g) * 2 + 0.3
    u = torch.randn(B, D, generator=g)
    mean, rstd = torch.randn(D, generator=g) * 0.3, torch.rand(D, generator=g) + 0.5
    w, beta = torch.randn(D, generator=g) * 0.5 + 1, torch.randn(D, generator=g) * 0.2
    return z, u, mean, rstd, w, beta


def _tail_bufs(z, u, mean, rstd, w, beta):
    return [_Buf(*t.shape, data=t) if t.dim() == 2 else _Buf(1, t.shape[0], data=t[None]) for t in (z, u, mean, rstd, w, beta)]


def test_tail_supported_predicates():
    L = _L().lib()
    for D in range(0, 300):
        assert int(L.sbr_bn_score_supported(D)) == int(D in TAIL_DS), D
        for N in (0, 1, 2, 16, 17):
            assert int(L.sbr_bn_score_loss_supported(D, N)) == int(D in TAIL_DS and 1 <= N <= min(16, D // 4)), (D, N)
    for C in range(0, 1100):
        assert int(L.sbr_act_grad_colsum_supported(C)) == int(C in (4, 8, 16, 32, 64, 128, 256, 512, 1024)), C


def _fwd_cases():
    cases = []
    for D in TAIL_DS:
        spb = 4 * (64 // (16 if D <= 64 else (32 if D <= 128 else 64)))       # slots per block of 4 waves
        cases += [(1, 1, D), (spb - 1, 1, D), (spb, 1, D), (spb + 1, 1, D), (7, 3, D), (37, 11, D)]   # N = 3 / 11: s / N changes inside a wave
    return cases


@pytest.mark.parametrize('B,N,D', _fwd_cases())
def test_bn_score_fwd(B, N, D):
    """sbr_bn_score_fwd on every supported D (LPS = 16 for D <= 64 — mostly idle lanes below 64 —, 32 for 128, 64 for 256), slot counts
    around the slots of a block, user boundaries inside a wave."""
    z, u, mean, rstd, w, beta = tail_input(B, N, D, 31 * D + B)
    bz, bu, bm, br, bw, bb = _tail_bufs(z, u, mean, rstd, w, beta)
    out = _Buf(1, B * N, off=0)
    call('sbr_bn_score_fwd', bz.ptr, bu.ptr, bm.ptr, br.ptr, bw.ptr, bb.ptr, out.ptr, B, N, D, stream())
    args = [_dd(t) for t in (z, u, mean, rstd, w, beta)]
    ref, _, _ = ref_score(*args, N)
    _assert_bound(out.check_untouched(None, 'logits')[0].view(B, N), ref, score_bound(*args, N), 'logits')


@pytest.mark.parametrize('D', [12, 24, 48, 96, 100, 192, 260])
def test_tail_refuses_unsupported_widths(D):
    z, u, mean, rstd, w, beta = tail_input(4, 2, D, 1)
    bz, bu, bm, br, bw, bb = _tail_bufs(z, u, mean, rstd, w, beta)
    out, g, du, dx = _Buf(1, 8), _Buf(4, 2, fill=1.0), _Buf(4, D), _Buf(8, D)
    ws = _zeros64(34 * D)
    st = stream()
    assert 'not supported' in _err('sbr_bn_score_fwd', bz.ptr, bu.ptr, bm.ptr, br.ptr, bw.ptr, bb.ptr, out.ptr, 4, 2, D, st)
    assert 'not supported' in _err('sbr_bn_score_bwd_stats', g.ptr, bu.ptr, bz.ptr, du.ptr, 4, 2, D, bw.ptr, bb.ptr, bm.ptr, br.ptr, _p(ws), st)
    assert 'not supported' in _err('sbr_bn_score_bwd_apply', g.ptr, bu.ptr, bz.ptr, dx.ptr, 4, 2, D, bw.ptr, bm.ptr, br.ptr, _p(ws), du.ptr, du.ptr, None, st)
    lws = _zeros64(int(_L().lib().sbr_bn_score_loss_workspace()) // 8)
    lab = _zeros64(8)
    assert 'not supported' in _err('sbr_bn_score_loss_fwd_bwd', bz.ptr, bu.ptr, bm.ptr, br.ptr, bw.ptr, bb.ptr, 0, _p(lab), 1.0, 0.0, None, out.ptr,
                                   du.ptr, _p(lab), None, 4, 2, D, _p(ws), _p(lws), lws.numel() * 8, st)
    out.check_untouched([], 'refused')
    du.check_untouched([], 'refused')
    dx.check_untouched([], 'refused')


def test_tail_refuses_each_misaligned_operand():
    B, N, D = 4, 2, 64
    z, u, mean, rstd, w, beta = tail_input(B, N, D, 2)
    ts = dict(z=z, u=u, mean=mean[None], rstd=rstd[None], w=w[None], beta=beta[None])
    st = stream()
    ws = _zeros64(34 * D)
    lws = _zeros64(int(_L().lib().sbr_bn_score_loss_workspace()) // 8)
    lab = _zeros64(B * N)
    for bad in list(ts) + ['du', 'dx']:
        b = {k: _Buf(*t.shape, off=1 if k == bad else 0, data=t) for k, t in ts.items()}
        out, g = _Buf(1, B * N), _Buf(B, N, fill=1.0)
        du, dx = _Buf(B, D, off=1 if bad == 'du' else 0), _Buf(B * N, D, off=1 if bad == 'dx' else 0)
        if bad not in ('du', 'dx'):
            assert 'not supported' in _err('sbr_bn_score_fwd', b['z'].ptr, b['u'].ptr, b['mean'].ptr, b['rstd'].ptr, b['w'].ptr, b['beta'].ptr, out.ptr, B, N, D, st)
        if bad != 'dx':
            assert 'not supported' in _err('sbr_bn_score_bwd_stats', g.ptr, b['u'].ptr, b['z'].ptr, du.ptr, B, N, D, b['w'].ptr, b['beta'].ptr,
                                           b['mean'].ptr, b['rstd'].ptr, _p(ws), st)
            assert 'not supported' in _err('sbr_bn_score_loss_fwd_bwd', b['z'].ptr, b['u'].ptr, b['mean'].ptr, b['rstd'].ptr, b['w'].ptr, b['beta'].ptr, 0,
                                           _p(lab), 1.0, 0.0, None, out.ptr, du.ptr, _p(lab), None, B, N, D, _p(ws), _p(lws), lws.numel() * 8, st)
        if bad not in ('du', 'beta'):
            assert 'not supported' in _err('sbr_bn_score_bwd_apply', g.ptr, b['u'].ptr, b['z'].ptr, dx.ptr, B, N, D, b['w'].ptr, b['mean'].ptr,
                                           b['rstd'].ptr, _p(ws), out.ptr, out.ptr, None, st)
        for t in (out, du, dx):
            t.check_untouched([], f'refused ({bad})')


def _pass_a_cases():
    cases = []
    for q, D in enumerate(TAIL_DS):
        RL = 256 // (D // 4)
        N = (1, 2, 11, 16, 17, 40, 3)[q]
        cases += [(1, N, D), (2 * RL - 1, N, D), (2 * RL, N, D), (2 * RL + 1, (2, 11, 16, 17, 40, 1, 5)[q], D)]
    cases += [(512 * 2 * 8 + 5, 3, 128), (512 * 2 * 16 + 1, 2, 64), (700, 17, 128), (300, 40, 256)]      # above the 512-block cap; N > 16
    return cases


@pytest.mark.parametrize('B,N,D', _pass_a_cases())
def test_bn_score_bwd_stats_and_apply(B, N, D):
    """Pass A (sbr_bn_score_bwd_stats): dU and the BatchNorm column sums against float64, with dU = NULL the same sums, replicas zeroed.
    Pass B (sbr_bn_score_bwd_apply) on the float64 totals of pass A as its given input: dX, dW / dBeta published once (= (float)ws),
    without ws_colsum and with it (the folded column sums of dX, finished by sbr_colred_finish: the kernel's own dX values summed, m
    fp32 additions per thread, then double, one final rounding)."""
    z, u, mean, rstd, w, beta = tail_input(B, N, D, 17 * D + B + N)
    g = _rand(B, N, seed=B + N)
    bz, bu, bm, br, bw, bb = _tail_bufs(z, u, mean, rstd, w, beta)
    G = _Buf(B, N, data=g)
    args = [_dd(t) for t in (g, u, z, mean, rstd, w, beta)]
    du_ref, s1, s2 = ref_pass_a(*args)
    bdu, b1, b2 = pass_a_bound(*args)
    ws = _zeros64(34 * D)
    st = stream()
    for with_du in (True, False, True):
        dU = _Buf(B, D)
        call('sbr_bn_score_bwd_stats', G.ptr, bu.ptr, bz.ptr, dU.ptr if with_du else None, B, N, D, bw.ptr, bb.ptr, bm.ptr, br.ptr, _p(ws), st)
        assert bool((ws[2 * D:] == 0).all()), 'replicas not zeroed'
        _assert_bound(ws[:D].cpu(), s1, b1, 'sum dy')
        _assert_bound(ws[D:2 * D].cpu(), s2, b2, 'sum dy xhat')
        if with_du:
            _assert_bound(dU.check_untouched(None, 'dU'), du_ref, bdu, 'dU')
        else:
            dU.check_untouched([], 'dU = NULL')
    tot = torch.cat([s1, s2])
    totd = tot.to(DEV)
    a7 = [_dd(t) for t in (g, u, z, mean, rstd, w)]
    dx_ref, dx_b = ref_pass_b(*a7, tot), pass_b_bound(*a7, tot)
    R = B * N
    m = colred_terms_per_thread(R, D)
    ws2 = _zeros64(17 * D)
    for colsum in (False, True, True):
        dX, dW, dBeta = _Buf(R, D), _Buf(1, D), _Buf(1, D)
        call('sbr_bn_score_bwd_apply', G.ptr, bu.ptr, bz.ptr, dX.ptr, B, N, D, bw.ptr, bm.ptr, br.ptr, _p(totd), dW.ptr, dBeta.ptr,
             _p(ws2) if colsum else None, st)
        _assert_bound(dX.check_untouched(None, 'dX'), dx_ref, dx_b, 'dX')
        _assert_bits(dW.check_untouched(None, 'dW')[0], s2.float(), 'dW = (float)ws')
        _assert_bits(dBeta.check_untouched(None, 'dBeta')[0], s1.float(), 'dBeta = (float)ws')
        if colsum:
            out = _Buf(1, D)
            wsa, outa, ca = (ctypes.c_void_p * 1)(ws2.data_ptr()), (ctypes.c_void_p * 1)(out.ptr), (ctypes.c_int * 1)(D)
            call('sbr_colred_finish', 1, ctypes.cast(wsa, ctypes.c_void_p), ctypes.cast(outa, ctypes.c_void_p), ctypes.cast(ca, ctypes.c_void_p), st)
            assert bool((ws2[D:] == 0).all())
            cs = dx_ref.sum(0)
            _assert_bound(out.check_untouched(None, 'colsum dX')[0], cs, dx_b.sum(0) + (m + 1) * U32 * dx_ref.abs().sum(0) + U32 * cs.abs(), 'colsum dX')


def _loss_cases():
    cases = []
    for N in range(1, 17):
        Dmin = next(D for D in TAIL_DS if N <= D // 4)
        for D in sorted({Dmin, 128} if N <= 32 else {Dmin}):
            for kind in (0, 1, 2):
                cases.append((kind, N, D))
    return cases


@pytest.mark.parametrize('kind,N,D', _loss_cases())
def test_bn_score_loss_fwd_bwd_against_float64(kind, N, D):
    """All 16 x 3 instantiations of bn_score_loss_kernel, each at the smallest D with N <= D / 4 and at D = 128, B in {1, 2 RL - 1,
    2 RL + 1, one above 512 * 2 * RL}: logits (bound of the forward), dlogits (the loss bound with the logits' own error propagated),
    dU and the column sums (pass A's bounds evaluated at the REFERENCE dlogits + the propagated dlogits error), the loss, out3, with
    logits = NULL and out3 = NULL in turn, workspaces left zeroed."""
    RL = 256 // (D // 4)
    L = _L().lib()
    st = stream()
    for B in (1, 2 * RL - 1, 2 * RL + 1, 512 * 2 * RL + 1):
        z, u, mean, rstd, w, beta = tail_input(B, N, D, 13 * D + B + N + kind)
        z, u = z * 0.5, u * (2.0 / math.sqrt(D))
        lab = torch.zeros(B, N, dtype=torch.float64)
        lab[:, 0] = 1
        if kind == 0:
            lab = torch.rand(B, N, generator=torch.Generator().manual_seed(B), dtype=torch.float64)     # soft labels
        cnt = {0: B * N, 1: B * max(N - 1, 1), 2: B}[kind]
        scale, shift = (1.0 / cnt if B % 2 else 1.0), (math.log(5000 / 10) if kind == 2 else 0.0)
        shift32 = float(np.float32(shift))
        bz, bu, bm, br, bw, bb = _tail_bufs(z, u, mean, rstd, w, beta)
        a6 = [_dd(t) for t in (z, u, mean, rstd, w, beta)]
        lg_ref, _, _ = ref_score(*a6, N)
        lg_b = score_bound(*a6, N)
        loss_ref, dl_ref = ref_rec_loss(kind, lg_ref, lab, scale, shift32)
        loss_b, dl_b = rec_loss_bounds(kind, lg_ref, lab, scale, shift32, ex=lg_b)
        du_ref, s1, s2 = ref_pass_a(dl_ref, *[a6[i] for i in (1, 0, 2, 3, 4, 5)])
        bdu, b1, b2 = pass_a_bound(dl_ref, *[a6[i] for i in (1, 0, 2, 3, 4, 5)])
        # the kernel's dlogits differ from the reference's by at most dl_b: that error goes linearly through dU and the column sums
        _, _, xh = ref_score(*a6, N)
        yabs = (xh * a6[4]).abs() + a6[5].abs()
        bdu = bdu + torch.einsum('bn,bnd->bd', dl_b, yabs) * (1 + 1e-3)
        e_dy = dl_b[:, :, None] * a6[1].abs()[:, None, :]
        b1, b2 = b1 + e_dy.sum((0, 1)) * (1 + 1e-3), b2 + (e_dy * xh.abs()).sum((0, 1)) * (1 + 1e-3)
        ws, lws, labd = _zeros64(34 * D), _zeros64(int(L.sbr_bn_score_loss_workspace()) // 8), lab.to(DEV)
        for rep in range(2):
            lg, dl, dU = _Buf(B, N), _Buf(B, N), _Buf(B, D)
            lo, o3 = torch.full((1,), 9.0, device=DEV, dtype=torch.float64), torch.full((3,), 9.0, device=DEV, dtype=torch.float64)
            call('sbr_bn_score_loss_fwd_bwd', bz.ptr, bu.ptr, bm.ptr, br.ptr, bw.ptr, bb.ptr, kind, _p(labd), scale, shift, lg.ptr if rep == 0 else None,
                 dl.ptr, dU.ptr, _p(lo), _p(o3) if rep == 0 else None, B, N, D, _p(ws), _p(lws), lws.numel() * 8, st)
            what = f'kind {kind} N {N} D {D} B {B}'
            if rep == 0:
                _assert_bound(lg.check_untouched(None, 'logits'), lg_ref, lg_b, 'logits ' + what)
                assert o3.cpu().tolist() == [float(lo), float(lo), 0.0]
            else:
                lg.check_untouched([], 'logits = NULL')
                assert o3.cpu().tolist() == [9.0, 9.0, 9.0]
            _assert_bound(dl.check_untouched(None, 'dlogits'), dl_ref, dl_b, 'dlogits ' + what)
            _assert_bound(dU.check_untouched(None, 'dU'), du_ref, bdu, 'dU ' + what)
            _assert_bound(ws[:D].cpu(), s1, b1, 'sum dy ' + what)
            _assert_bound(ws[D:2 * D].cpu(), s2, b2, 'sum dy xhat ' + what)
            assert abs(float(lo) - float(loss_ref)) <= float(loss_b), (what, float(lo), float(loss_ref), float(loss_b))
            assert bool((ws[2 * D:] == 0).all()) and int(lws.view(torch.int64)[0]) == 0      # replicas zeroed, arrival counter reset
            if kind == 1 and N == 1:
                assert float(lo) == 0.0 and bool((dl.host() == 0).all())


# ---- sbr_act_grad_gather_colsum / sbr_colred_finish --------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [4, 8, 64, 128, 256, 512, 1024])
@pytest.mark.parametrize('act', [1, 2, 3, 4])
def test_act_grad_gather_colsum(C, act):
    """dZ[j] = dY[ii(j)] act'(Y[ii(j)]) (one product: |dY| e_g + u |dZ|) with duplicate source rows, ld > C, ldz > C, n around the block
    quantum and above the 512-block cap; the pending column sums finished by sbr_colred_finish: sum of the kernel's dZ, m fp32
    additions per thread, double after that, one rounding at the end. Y = act(pre) holds exact zeros for relu (act' = 0 there)."""
    RL = 256 // (C // 4)
    for n, use_idx in ((1, False), (8 * RL - 1, True), (8 * RL + 1, False), (512 * 8 * RL + 3 if C <= 128 else 16 * RL + 3, True)):
        n_src = n if not use_idx else max(3, n // 2)
        pre = _rand(n_src, C, seed=C + n)
        y, dy = ref_act(_dd(pre), act).float(), _rand(n_src, C, seed=C + n + 1)
        Yb, dYb = _Buf(n_src, C, ld=C + 8, data=y), _Buf(n_src, C, ld=C + 8, data=dy)
        idx = np.random.default_rng(n).integers(0, n_src, size=n) if use_idx else None
        idx_d = torch.as_tensor(idx, dtype=torch.int32).to(DEV) if use_idx else None
        dZ, ws, out = _Buf(n, C, ld=C + 4), _zeros64(17 * C), _Buf(1, C)
        call('sbr_act_grad_gather_colsum', dYb.ptr, Yb.ptr, C + 8, _p(idx_d), dZ.ptr, C + 4, n, C, act, _p(ws), stream())
        src = torch.as_tensor(idx if use_idx else np.arange(n))
        yd, dyd = _dd(y)[src], _dd(dy)[src]
        ref = dyd * ref_act_grad_from_out(yd, act)
        bz = dyd.abs() * act_grad_err(yd, act) + U32 * ref.abs()
        _assert_bound(dZ.check_untouched(None, 'dZ'), ref, bz, f'dZ act {act}')
        wsa, outa, ca = (ctypes.c_void_p * 1)(ws.data_ptr()), (ctypes.c_void_p * 1)(out.ptr), (ctypes.c_int * 1)(C)
        call('sbr_colred_finish', 1, ctypes.cast(wsa, ctypes.c_void_p), ctypes.cast(outa, ctypes.c_void_p), ctypes.cast(ca, ctypes.c_void_p), stream())
        m = colred_terms_per_thread(n, C)
        cs = ref.sum(0)
        _assert_bound(out.check_untouched(None, 'colsum')[0], cs, bz.sum(0) + (m + 1) * U32 * ref.abs().sum(0) + U32 * cs.abs(), 'colsum dZ')
        assert bool((ws[C:] == 0).all())


@pytest.mark.parametrize('C', [12, 100, 1028])
def test_act_grad_gather_colsum_refuses(C):
    t, ws, dz = torch.zeros(4 * C + 8, device=DEV), _zeros64(17 * C), _Buf(2, C)
    assert 'not supported' in _err('sbr_act_grad_gather_colsum', _p(t), _p(t), C, None, dz.ptr, C, 2, C, 1, _p(ws), stream())
    dz.check_untouched([], 'refused')
    t64 = torch.zeros(600, device=DEV)
    dz = _Buf(2, 64)
    for args in ((t64.data_ptr() + 4, _p(t64), 64, dz.ptr, 64), (_p(t64), t64.data_ptr() + 8, 64, dz.ptr, 64), (_p(t64), _p(t64), 66, dz.ptr, 64),
                 (_p(t64), _p(t64), 64, dz.ptr, 66), (_p(t64), _p(t64), 64, dz.ptr + 4, 64)):
        assert 'not supported' in _err('sbr_act_grad_gather_colsum', args[0], args[1], args[2], None, args[3], args[4], 2, 64, 1, _p(_zeros64(17 * 64)), stream())
    dz.check_untouched([], 'refused')


def test_colred_finish_counts_and_widths():
    """count 0 (nothing), 1, 8 reductions of DIFFERENT widths in one launch (out[q][c] = sum over the 16 replicas of workspaces[q],
    rounded once; replicas zeroed; the totals part [0, C) of a workspace is not touched), 9 refused."""
    widths = [4, 300, 64, 1, 1024, 128, 12, 257]
    call('sbr_colred_finish', 0, None, None, None, stream())
    for count in (1, 8):
        wss, outs, refs = [], [], []
        for q in range(count):
            C = widths[q]
            w = torch.randn(17, C, generator=torch.Generator().manual_seed(q), dtype=torch.float64)
            w[0] = 123.0
            refs.append(w[1:].sum(0))
            wss.append(w.to(DEV))
            outs.append(_Buf(1, C))
        wsa, outa = (ctypes.c_void_p * count)(*[w.data_ptr() for w in wss]), (ctypes.c_void_p * count)(*[o.ptr for o in outs])
        ca = (ctypes.c_int * count)(*widths[:count])
        call('sbr_colred_finish', count, ctypes.cast(wsa, ctypes.c_void_p), ctypes.cast(outa, ctypes.c_void_p), ctypes.cast(ca, ctypes.c_void_p), stream())
        for q in range(count):
            mag = wss[q].cpu()                                 # (already zeroed: use the reference's magnitudes)
            assert bool((mag[1:] == 0).all()) and bool((mag[0] == 123.0).all())
            _assert_bound(outs[q].check_untouched(None, f'out {q}')[0], refs[q], U32 * refs[q].abs() + 16 * U64 * 16, f'colred_finish {q} of {count}')
    p9 = (ctypes.c_void_p * 9)(*([wss[0].data_ptr()] * 9))
    c9 = (ctypes.c_int * 9)(*([4] * 9))
    assert '1..8' in _err('sbr_colred_finish', 9, ctypes.cast(p9, ctypes.c_void_p), ctypes.cast(p9, ctypes.c_void_p), ctypes.cast(c9, ctypes.c_void_p), stream())


def test_pack_losses():
    rec, ra, rb = [torch.tensor([v], dtype=torch.float64, device=DEV) for v in (1.25, 0.5, -3.0)]
    for a in (None, ra):
        for b in (None, rb):
            out = torch.full((3,), NAN, dtype=torch.float64, device=DEV)
            call('sbr_pack_losses', _p(rec), _p(a), 0.1, _p(b), 0.01, _p(out), stream())
            reg = (0.1 * 0.5 if a is not None else 0.0) + (0.01 * -3.0 if b is not None else 0.0)
            assert out.cpu().tolist() == [1.25 + reg, 1.25, reg]
    assert 'null operand' in _err('sbr_pack_losses', None, None, 0.0, None, 0.0, _p(rec), stream())


# =================================================================================================================================
# recommendation losses
# =================================================================================================================================
def loss_logits(B, N, seed):
    """randn * 3, with rows that hold +-30 and +-90 (and, for the float64 losses, +-1e4 — see the test)"""
    x = _rand(max(B, 1), N, seed=seed)[:B] * 3
    for r, v in enumerate((30.0, -30.0, 90.0, -90.0)):
        if r < B:
            x[r, r % N] = v
            x[r, (r + 1) % N] = -v if N > 1 else v
    return x


def _rec_loss_cases():
    """every kind x B x N, the large batch at two widths only (suite time; the smaller B cover every N)"""
    return [(kind, B, N) for kind in (0, 1, 2) for B in (0, 1, 255, 256, 257, 100000) for N in (1, 2, 11, 16) if B < 100000 or N in (2, 11)]


@pytest.mark.parametrize('kind,B,N', _rec_loss_cases())
def test_rec_losses_against_float64(kind, B, N, det):
    """sbr_rec_loss_fwd, _bwd (float and double grad_out), _fwd_bwd, _fwd_bwd_ws. BCE / BPR: loss to 1e-12 relative to sum|terms|
    (double arithmetic; the order of the block sums only permutes a double sum), dlogits within half an fp32 ulp of the float64 gradient
    (BPR: on the fp32 difference x0 - xj the reference takes too); rows with +-1e4 included; BCE with soft labels. Sampled softmax: the
    derived fp32 bound, shifts 0, 0.37 and log(50000 / 10). N = 1: BPR loss 0 and a zero gradient, sampled-softmax loss 0.
    Deterministic mode: sbr_rec_loss_fwd / _fwd_bwd take their fixed-order forms (same bounds, loss and dlogits of two calls
    bit-identical); _bwd and _fwd_bwd_ws have no arrival-order accumulation and run as they are."""
    for _ in (0,):
        x = loss_logits(B, N, 100 * N + kind)
        if kind != 2 and B > 5:
            x[4, 0], x[5, N - 1] = 1e4, -1e4
        if kind == 0:
            lab = torch.rand(B, N, generator=torch.Generator().manual_seed(B + N), dtype=torch.float64)
            lab[:, 0] = 1
        else:
            lab = torch.zeros(B, N, dtype=torch.float64)
            lab[:, 0] = 1
        xd, labd = (x if B else torch.zeros(1, N)).to(DEV), (lab if B else torch.zeros(1, N, dtype=torch.float64)).to(DEV)      # B = 0: non-null pointers
        st = stream()
        for shift in ((0.0, 0.37, math.log(50000 / 10)) if kind == 2 else (0.0,)):
            for mean in (True, False):
                cnt = {0: B * N, 1: B * (N - 1), 2: B}[kind]
                scale = 1.0 / cnt if (mean and cnt) else 1.0
                shift32 = float(np.float32(shift))
                loss_ref, dl_ref = ref_rec_loss(kind, _dd(x), lab, scale, shift32)
                bl, bdl = rec_loss_bounds(kind, _dd(x), lab, scale, shift32)
                what = f'kind {kind} B {B} N {N} shift {shift} mean {mean}'
                lo = torch.full((1,), 7.0, dtype=torch.float64, device=DEV)
                fwd_seen = []
                for rep in range(2):
                    lo.fill_(7.0)
                    call('sbr_rec_loss_fwd', kind, _p(xd), _p(labd), B, N, scale, shift, _p(lo), st)
                    assert abs(float(lo) - float(loss_ref)) <= float(bl), (what, float(lo), float(loss_ref), float(bl))
                    fwd_seen.append((lo.cpu().clone(),))
                _same_bits(det, [(t[0].view(torch.int32),) for t in fwd_seen], 'sbr_rec_loss_fwd')
                if N == 1 and kind in (1, 2):
                    assert float(lo) == 0.0 or kind == 2 and abs(float(lo)) <= float(bl)
                for gval, is_double in ((1.0, 0), (-2.5, 0), (0.75, 1)):
                    gout = torch.tensor([gval], dtype=torch.float64 if is_double else torch.float32, device=DEV)
                    dl = _Buf(max(B, 1), N)
                    call('sbr_rec_loss_bwd', kind, _p(xd), _p(labd), B, N, scale, shift, _p(gout), is_double, dl.ptr, st)
                    got = dl.check_untouched(torch.arange(B), 'dlogits')[:B]
                    r2, b2 = ref_rec_loss(kind, _dd(x), lab, scale * gval, shift32)[1], rec_loss_bounds(kind, _dd(x), lab, abs(scale * gval), shift32)[1]
                    _assert_bound(got, r2, b2, 'bwd ' + what)
                fb_seen = []
                for rep in range(2):
                    dl = _Buf(max(B, 1), N)
                    lo.fill_(7.0)
                    call('sbr_rec_loss_fwd_bwd', kind, _p(xd), _p(labd), B, N, scale, shift, _p(lo), dl.ptr, st)
                    assert abs(float(lo) - float(loss_ref)) <= float(bl), what
                    g0 = dl.check_untouched(torch.arange(B), 'dlogits')[:B]
                    _assert_bound(g0, dl_ref, bdl, 'fwd_bwd ' + what)
                    fb_seen.append((lo.cpu().view(torch.int32).clone(), g0))
                _same_bits(det, fb_seen, 'sbr_rec_loss_fwd_bwd')
                if N == 1 and kind == 1:
                    assert float(lo) == 0.0 and bool((g0 == 0).all())
                if B >= 1:
                    need = int(_L().lib().sbr_rec_loss_workspace(B))
                    ws = _zeros64(need // 8)
                    dl2, o3 = _Buf(B, N), torch.full((3,), 9.0, dtype=torch.float64, device=DEV)
                    lo.fill_(-1.0)
                    call('sbr_rec_loss_fwd_bwd_ws', kind, _p(xd), _p(labd), B, N, scale, shift, _p(lo), dl2.ptr, _p(o3), _p(ws), need, st)
                    assert abs(float(lo) - float(loss_ref)) <= float(bl), what
                    assert o3.cpu().tolist() == [float(lo), float(lo), 0.0] and int(ws.view(torch.int64)[0]) == 0      # arrival counter reset
                    _assert_bits(dl2.check_untouched(None, 'dlogits ws'), g0, 'fwd_bwd_ws dlogits')
                else:
                    assert 'empty batch' in _err('sbr_rec_loss_fwd_bwd_ws', kind, _p(xd), _p(labd), 0, N, scale, shift, _p(lo), dl.ptr, None, _p(lo), 8, st)
    assert 'unknown loss kind' in _err('sbr_rec_loss_fwd', 3, _p(torch.zeros(4, device=DEV)), None, 1, 1, 1.0, 0.0, _p(_zeros64(1)), stream())


# =================================================================================================================================
# InfoNCE
# =================================================================================================================================
def _infonce_cases():
    cases = []
    for q, N in enumerate((1, 15, 16, 17, 32, 33, 176)):
        D = (3, 4, 64, 128, 256, 260, 64)[q]
        G = (1, 15, 16, 17, 5, 3, 1)[q]
        cases.append((G, N, D, (1.0, 0.3, 0.05)[q % 3], q % 2 == 1, False, 0))
    cases += [(1027, 11, 128, 0.3, False, True, 0),          # the training step's call: in-place ld = 2 D slices
              (17, 16, 256, 0.05, True, True, 0), (9, 16, 64, 1.0, True, False, 1),      # A 4 bytes off: the generic kernel at a small-kernel shape
              (16, 2, 4, 0.05, True, False, 0), (4, 16, 260, 0.3, False, False, 0), (2, 40, 3, 0.3, True, False, 0)]
    return cases


@pytest.mark.parametrize('G,N,D,tau,normalise,inplace,off', _infonce_cases())
def test_infonce_lds_routes_against_float64(G, N, D, tau, normalise, inplace, off, det):
    """sbr_infonce_fwd / _bwd: the one-wave kernel (N <= 16, D <= 256, D % 4 == 0, aligned) and the one-workgroup kernel on both sides of
    N = 16 | 17, D = 256 | 260, D % 4, alignment; N = 176 (more than 64 KB of LDS); tau down to 0.05 on L2-normalised rows (logits up to
    20) and on raw randn * 0.5 rows; `ld = 2 D` slices read and written in place. Deterministic mode: the forward adds its workgroup
    partial sums in a fixed pattern (same bound, two calls bit-identical); the backward has no accumulation across threads."""
    a, b = _rand(G, N, D, seed=G + N) * 0.5, _rand(G, N, D, seed=G + N + 1) * 0.5
    if normalise:
        a, b = torch.nn.functional.normalize(a, dim=-1), torch.nn.functional.normalize(b, dim=-1)
    scale = 1.0 / (G * N) if G % 2 else 1.0
    ld = 2 * D if inplace else D
    if inplace:
        E = _Buf(G * N, 2 * D, data=torch.cat([a.reshape(G * N, D), b.reshape(G * N, D)], 1))
        pa, pb = E.ptr, E.ptr + 4 * D
        dE = _Buf(G * N, 2 * D)
        pda, pdb = dE.ptr, dE.ptr + 4 * D
    else:
        A, Bb = _Buf(G * N, D, off=off, data=a.reshape(G * N, D)), _Buf(G * N, D, data=b.reshape(G * N, D))
        dA, dB = _Buf(G * N, D), _Buf(G * N, D)
        pa, pb, pda, pdb = A.ptr, Bb.ptr, dA.ptr, dB.ptr
    loss_ref, da_ref, db_ref, _, _ = ref_infonce(_dd(a), _dd(b), float(np.float32(tau)), scale)
    bl, bA, bB = infonce_bounds(_dd(a), _dd(b), float(np.float32(tau)), scale)
    lo = torch.full((1,), 5.0, dtype=torch.float64, device=DEV)
    gout = torch.ones(1, device=DEV)
    seen = []
    for rep in range(2):
        lo.fill_(5.0)
        call('sbr_infonce_fwd', pa, pb, ld, G, N, D, tau, scale, _p(lo), stream())
        assert abs(float(lo) - float(loss_ref)) <= float(bl), (float(lo), float(loss_ref), float(bl))
        for t in ((dE,) if inplace else (dA, dB)):
            t.flat.fill_(NAN)
        call('sbr_infonce_bwd', pa, pb, ld, G, N, D, tau, scale, _p(gout), pda, pdb, ld, stream())
        if inplace:
            got = dE.check_untouched(None, 'dE')
            ga, gb = got[:, :D], got[:, D:]
        else:
            ga, gb = dA.check_untouched(None, 'dA'), dB.check_untouched(None, 'dB')
        seen.append((lo.cpu().view(torch.int32).clone(), ga.contiguous(), gb.contiguous()))
    _same_bits(det, seen, 'sbr_infonce_fwd / _bwd')
    # up = gout * (float)scale * inv_tau in fp32: three roundings relative to the gradient itself
    _assert_bound(ga.reshape(G, N, D), da_ref, bA + 3 * U32 * da_ref.abs(), 'dA')
    _assert_bound(gb.reshape(G, N, D), db_ref, bB + 3 * U32 * db_ref.abs(), 'dB')


def test_infonce_route_choice_and_refusal():
    ops = S().ops
    assert ops.infonce_max_n() == 176
    assert not ops.infonce_uses_gemm(32, 176) and ops.infonce_uses_gemm(1, 177) and ops.infonce_uses_gemm(5000, 177)
    assert ops.infonce_uses_gemm(1, 176)                      # few large groups: the GEMM route although the LDS entry would take them
    assert not ops.infonce_uses_gemm(32, 33) and ops.infonce_uses_gemm(31, 33) and not ops.infonce_uses_gemm(1, 32)
    t, lo = torch.zeros(177 * 8, device=DEV), _zeros64(1)
    assert 'outside [1, 176]' in _err('sbr_infonce_fwd', _p(t), _p(t), 4, 1, 177, 4, 0.3, 1.0, _p(lo), stream())
    assert 'outside [1, 176]' in _err('sbr_infonce_bwd', _p(t), _p(t), 4, 1, 177, 4, 0.3, 1.0, _p(t), _p(t), _p(t), 4, stream())
    assert 'outside [1, 176]' in _err('sbr_infonce_fwd', _p(t), _p(t), 4, 1, 0, 4, 0.3, 1.0, _p(lo), stream())


@pytest.mark.parametrize('G,N,D,tau', [(1, 177, 64, 0.3), (2, 33, 128, 0.05), (1, 300, 30, 1.0)])
def test_infonce_gemm_route_against_float64(G, N, D, tau, det):
    """N = 177 (refused by the LDS entry) and N = 33 with few groups go through ops to sbr_infonce_gemm_fwd / _bwd: the bounds of
    infonce_bounds as they are (see there why the GEMM route has the same rounding counts). Deterministic mode: the forward's loss
    scalar is an arrival-order sum ("no deterministic form"); the backward has none and gives the same bits twice."""
    ops = S().ops
    assert ops.infonce_uses_gemm(G, N)
    a, b = torch.nn.functional.normalize(_rand(G, N, D, seed=N), dim=-1), torch.nn.functional.normalize(_rand(G, N, D, seed=N + 1), dim=-1)
    scale = 1.0 / (G * N)
    ad, bd = a.to(DEV).contiguous(), b.to(DEV).contiguous()
    lo = torch.full((), 3.0, dtype=torch.float64, device=DEV)
    loss_ref, da_ref, db_ref, _, _ = ref_infonce(_dd(a), _dd(b), float(np.float32(tau)), scale)
    bl, bA, bB = infonce_bounds(_dd(a), _dd(b), float(np.float32(tau)), scale)
    if det:
        with pytest.raises(_L().SibrarHipError, match='no deterministic form'):
            ops.infonce_fwd(ad.data_ptr(), bd.data_ptr(), D, G, N, D, tau, scale, lo, ad.device)
        assert float(lo) == 3.0
    else:
        ops.infonce_fwd(ad.data_ptr(), bd.data_ptr(), D, G, N, D, tau, scale, lo, ad.device)
        torch.cuda.synchronize()
        assert abs(float(lo) - float(loss_ref)) <= float(bl), (float(lo), float(loss_ref), float(bl))
    gout = torch.ones((), device=DEV)
    seen = []
    for rep in range(2):
        dA, dB = _Buf(G * N, D), _Buf(G * N, D)
        ops.infonce_bwd(ad.data_ptr(), bd.data_ptr(), D, G, N, D, tau, scale, gout, dA.ptr, dB.ptr, D, ad.device)
        torch.cuda.synchronize()
        ga, gb = dA.check_untouched(None, 'dA'), dB.check_untouched(None, 'dB')
        _assert_bound(ga.reshape(G, N, D), da_ref, bA + 3 * U32 * da_ref.abs(), 'dA (gemm)')
        _assert_bound(gb.reshape(G, N, D), db_ref, bB + 3 * U32 * db_ref.abs(), 'dB (gemm)')
        seen.append((ga, gb))
    _same_bits(det, seen, 'sbr_infonce_gemm_bwd')


# =================================================================================================================================
# deterministic mode
# =================================================================================================================================
def test_deterministic_mode_fixed_order_forms_and_refusals():
    """Under ops.set_deterministic(True): BatchNorm forward / backward (D = 128, 64), the recommendation loss and InfoNCE inside the
    default-mode bounds, two calls bit-identical, no arrival-order launch counted; D = 130 BatchNorm and the arrival-order-only entries
    raise "no deterministic form"."""
    ops, L = S().ops, _L().lib()
    prev = ops.set_deterministic(True)
    try:
        L.sbr_reset_nondeterministic_launches()
        st = stream()
        for n, D, act in ((4097, 128, 4), (70, 64, 2), (66000, 64, 1)):
            x, w, b = bn_input(n, D, 5 * D + n, act)
            xd = _dd(x)
            m, var, rstd = ref_bn_stats(xd)
            dm, dvar = bn_stats_err(xd, n)
            em, er = dm + U32 * m.abs(), 0.5 * dvar / (var + EPS32) + U32
            yref, yb = bn_fwd_bound(xd, _dd(w), _dd(b), m, rstd, act, em, er)
            X, wd_, bd_, ws = _Buf(n, D, data=x), w.to(DEV), b.to(DEV), _zeros64(34 * D)
            seen = []
            for rep in range(2):
                Y, sm_, sr_ = _Buf(n, D), _Buf(1, D), _Buf(1, D)
                call('sbr_bn_train_fwd', X.ptr, Y.ptr, n, D, _p(wd_), _p(bd_), None, None, None, sm_.ptr, sr_.ptr, _p(ws), EPS, MOM, act, st)
                y = Y.check_untouched(None, 'Y')
                _assert_bound(y, yref, yb, 'Y (deterministic)')
                _assert_bound(sr_.host()[0], rstd, rstd * er, 'rstd (deterministic)')
                seen.append((y, sm_.host(), sr_.host()))
            for p, q in zip(*seen):
                _assert_bits(p, q, 'BatchNorm forward, two deterministic calls')
            y32, m32, r32, dy = yref.float(), m.float(), rstd.float(), _rand(n, D, seed=3)
            dxr, dwr, dbr = ref_bn_bwd(_dd(dy), _dd(y32), xd, _dd(w), _dd(m32), _dd(r32), act)
            bx, bw, bb = bn_bwd_bound(_dd(dy), _dd(y32), xd, _dd(w), _dd(m32), _dd(r32), act)
            dYb, Yb, Mb, Rb = _Buf(n, D, data=dy), _Buf(n, D, data=y32), _Buf(1, D, data=m32[None]), _Buf(1, D, data=r32[None])
            seen = []
            for rep in range(2):
                dX, dW, dB = _Buf(n, D), _Buf(1, D), _Buf(1, D)
                call('sbr_bn_train_bwd', dYb.ptr, Yb.ptr, X.ptr, dX.ptr, n, D, _p(wd_), Mb.ptr, Rb.ptr, dW.ptr, dB.ptr, _p(ws), act, st)
                _assert_bound(dX.check_untouched(None, 'dX'), dxr, bx, 'dX (deterministic)')
                _assert_bound(dW.host()[0], dwr, bw, 'dW (deterministic)')
                _assert_bound(dB.host()[0], dbr, bb, 'dB (deterministic)')
                seen.append((dX.host(), dW.host(), dB.host()))
            for p, q in zip(*seen):
                _assert_bits(p, q, 'BatchNorm backward, two deterministic calls')
        for kind in (0, 1, 2):
            B, N = 100000, 11
            x = loss_logits(B, N, kind)
            lab = torch.zeros(B, N, dtype=torch.float64)
            lab[:, 0] = 1
            loss_ref, dl_ref = ref_rec_loss(kind, _dd(x), lab, 1.0 / B, float(np.float32(0.37)) if kind == 2 else 0.0)
            bl, bdl = rec_loss_bounds(kind, _dd(x), lab, 1.0 / B, float(np.float32(0.37)) if kind == 2 else 0.0)
            xd_, labd = x.to(DEV), lab.to(DEV)
            vals = []
            for fn in ('sbr_rec_loss_fwd', 'sbr_rec_loss_fwd_bwd', 'sbr_rec_loss_fwd', 'sbr_rec_loss_fwd_bwd'):
                lo, dl = _zeros64(1), _Buf(B, N)
                extra = (dl.ptr,) if fn.endswith('bwd') else ()
                call(fn, kind, _p(xd_), _p(labd), B, N, 1.0 / B, 0.37 if kind == 2 else 0.0, _p(lo), *extra, st)
                assert abs(float(lo) - float(loss_ref)) <= float(bl)
                vals.append(float(lo))
            assert vals[0] == vals[2] and vals[1] == vals[3]
        for G, N, D in ((1027, 11, 128), (5, 40, 30)):
            a, b = _rand(G, N, D, seed=1) * 0.5, _rand(G, N, D, seed=2) * 0.5
            loss_ref = ref_infonce(_dd(a), _dd(b), float(np.float32(0.3)), 1.0 / (G * N))[0]
            bl = infonce_bounds(_dd(a), _dd(b), float(np.float32(0.3)), 1.0 / (G * N))[0]
            ad, bd = a.to(DEV), b.to(DEV)
            vals = []
            for rep in range(2):
                lo = _zeros64(1)
                call('sbr_infonce_fwd', _p(ad), _p(bd), D, G, N, D, 0.3, 1.0 / (G * N), _p(lo), st)
                assert abs(float(lo) - float(loss_ref)) <= float(bl)
                vals.append(float(lo))
            assert vals[0] == vals[1]
        assert int(L.sbr_nondeterministic_launches()) == 0
        # no fixed-order form
        t, ws = torch.zeros(130 * 8, device=DEV), _zeros64(34 * 130)
        assert 'no deterministic form' in _err('sbr_bn_train_fwd', _p(t), _p(t), 4, 130, _p(t), _p(t), None, None, None, _p(t), _p(t), _p(ws), EPS, MOM, 0, st)
        assert 'no deterministic form' in _err('sbr_bn_train_bwd', _p(t), _p(t), _p(t), _p(t), 4, 130, _p(t), _p(t), _p(t), _p(t), _p(t), _p(ws), 0, st)
        z, u, mean, rstd, w, beta = tail_input(4, 2, 64, 1)
        bz, bu, bm, br, bw_, bb_ = _tail_bufs(z, u, mean, rstd, w, beta)
        g, du, dx, lab = _Buf(4, 2, fill=1.0), _Buf(4, 64), _Buf(8, 64), _zeros64(8)
        ws, lws = _zeros64(34 * 64), _zeros64(int(L.sbr_bn_score_loss_workspace()) // 8)
        assert 'no deterministic form' in _err('sbr_bn_score_bwd_stats', g.ptr, bu.ptr, bz.ptr, du.ptr, 4, 2, 64, bw_.ptr, bb_.ptr, bm.ptr, br.ptr, _p(ws), st)
        assert 'no deterministic form' in _err('sbr_bn_score_loss_fwd_bwd', bz.ptr, bu.ptr, bm.ptr, br.ptr, bw_.ptr, bb_.ptr, 0, _p(lab), 1.0, 0.0, None, g.ptr,
                                               du.ptr, _p(lab), None, 4, 2, 64, _p(ws), _p(lws), lws.numel() * 8, st)
        assert 'no deterministic form' in _err('sbr_bn_score_bwd_apply', g.ptr, bu.ptr, bz.ptr, dx.ptr, 4, 2, 64, bw_.ptr, bm.ptr, br.ptr, _p(ws), du.ptr, du.ptr,
                                               _p(_zeros64(17 * 64)), st)
        call('sbr_bn_score_bwd_apply', g.ptr, bu.ptr, bz.ptr, dx.ptr, 4, 2, 64, bw_.ptr, bm.ptr, br.ptr, _p(ws), du.ptr, du.ptr, None, st)    # fixed order without ws_colsum
        t64 = torch.zeros(8 * 64, device=DEV)
        assert 'no deterministic form' in _err('sbr_act_grad_gather_colsum', _p(t64), _p(t64), 64, None, dx.ptr, 64, 4, 64, 1, _p(_zeros64(17 * 64)), st)
        wsb = torch.zeros(int(L.sbr_infonce_gemm_workspace(40, 64)), dtype=torch.uint8, device=DEV)
        tt = torch.zeros(40 * 64, device=DEV)
        assert 'no deterministic form' in _err('sbr_infonce_gemm_fwd', _p(tt), _p(tt), 64, 1, 40, 64, 0.3, 1.0, _p(lab), _p(wsb), wsb.numel(), st)
        assert int(L.sbr_nondeterministic_launches()) == 0
    finally:
        ops.set_deterministic(prev)
