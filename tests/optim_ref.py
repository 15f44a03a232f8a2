"""Float64 update rules, derived one-step error bounds and an fp32 restatement for the optimizer kernels (csrc/optim.hip). A plain module:
no fixtures, no pytest hooks, no GPU. tests/test_optim_refs_cpu.py shows on the CPU that the rules equal torch.optim, that the fp32
restatement stays inside the bounds on every input set of the GPU tests and that each listed wrong kernel leaves them;
tests/test_hip_optim.py applies rules and bounds to the kernels.

(a) Rules. torch.optim.AdamW / Adam / Adagrad, single-tensor form, on fp32 state promoted to float64 with the hyper-parameters as
Python doubles (bc1 = 1 - b1^step, bc2 = 1 - b2^step):
    AdamW  p1 = p (1 - lr wd),  g' = g                    Adam  p1 = p,  g' = g + wd p
    m' = m + (g' - m)(1 - b1)                             exp_avg.lerp_(grad, 1 - beta1)
    v' = v b2 + (1 - b2) g' g'                            exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    den = sqrt(v') / sqrt(bc2) + eps
    p' = p1 - (lr / bc1) (m' / den)                       param.addcdiv_(exp_avg, denom, value=-step_size)
    Adagrad  g' = g + wd p,  s' = s + g' g',  p' = p - lr (g' / (sqrt(s') + eps))        (lr_decay = 0)

(b) Bounds — derived, never fitted. u = 2^-24 (hip_testutil.U32), eta = 2^-150. One fp32 operation returns fl(x) = x (1 + d),
|d| <= u; a product, quotient or root whose result is subnormal adds an absolute eta (half the subnormal spacing), a sum or
difference does not (it is exact there). Every host-side scalar (1 - b1, b2, 1 - b2, 1 - lr wd, wd, lr / bc1, sqrt(bc2), eps) is
evaluated in double and rounded to fp32 once: one more factor (1 + d). sqrtf and the division are allowed one ulp (2 u) each, twice
what a correctly rounded one needs. The kernel's order is adam_element's, without contraction:
    p1^  = fl(p decay^)                                   e_p1 = 2 u |p1| + eta          (0 for Adam, and when lr wd = 0: decay = 1)
    g'^  = fl(g + fl(wd^ p))                              dg   = u |g'| + 2 u |wd p| + eta                              (0 for AdamW)
    m'^  = fl(m + fl(fl(g'^ - m) omb1^))                  the difference carries dg + u |g' - m|, the product two more roundings:
                                                          bm   = u |m'| + 3 u (1 - b1) |g' - m| + (1 - b1) dg + eta
    v'^  = fl(fl(v b2^) + fl(fl(omb2^ g'^) g'^))          with c = (1 - b2) g'^2:
                                                          bv   = u (v' + 2 b2 v + 3 c) + 2 (1 - b2) |g'| dg + (1 - b2) dg^2 + eta (2 + |g'|)
    s^   = sqrtf(v'^)                                     |sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b) <= sqrt |a - b|:
                                                          ds   = min(bv / (sqrt v' + sqrt max(v' - bv, 0)), sqrt bv),  ds += 2 u (s + ds)
    q^   = fl(s^ / bc2s^)                                 dq   = ds / sqrt(bc2) + 3 u q
    den^ = fl(q^ + eps^)                                  dden = dq + u eps + u den,      den_lo = den - dden (bound = inf unless > 0)
    r^   = fl(m'^ / den^)                                 dr   = bm / den_lo + |m'| dden / (den den_lo) + 2 u |r| + eta
    w^   = fl(ss^ r^)                                     dw   = (lr / bc1) (dr + 2 u |r|) + eta
    p'^  = fl(p1^ - w^)                                   bp   = e_p1 + dw + u |p'|
The starting point named in the issue that asked for this module had the same bm with |g' - m| <= |g'| + |m| and measured 0.97 of it
on an fp32 restatement: the first-order count is attained, so the slack is added explicitly. Every bound above is multiplied by
MARGIN = 1.125 and one fp32 subnormal (2^-149) is added. The eighth pays for what first order drops — products of two roundings
(relative 2^-20 of the bound at most), the float64 evaluation of reference and bound (2^-50) — with room to spare; it is not needed
by, and was not sized to, any measured kernel error. Incoming state errors (e_in = errors of p, m, v; for a replay over several
steps) propagate with the rule's own derivatives: |decay| e_p into p1, wd e_p into g' (Adam), b1 e_m into m', b2 e_v into v'.
adagrad_kernel has no contraction pragma: each a * b + c may round once (fma) or twice; the bound counts twice, which covers both:
    dg = u |g'| + 2 u |wd p| + eta;   bs = u (s' + g'^2) + 2 |g'| dg + dg^2 + eta;   ds, dden, dr, dw, bp as above with bc2 = 1, lr / bc1 = lr,
    the numerator g' (dg in place of bm) and e_p1 = 0.
Non-finite elements (a gradient of inf / NaN) have no bound (NaN): the tests compare their class and mask them.

(c) The fp32 restatement: numpy float32, one operation per line, adam_element's order, scalars rounded once from double. ``mutant``
turns it into one of the wrong kernels the bounds must reject (MUTANTS_ADAM / MUTANTS_ADAGRAD)."""
import math

import numpy as np
import torch

from hip_testutil import U32

ETA = 2.0 ** -150
TINY = 2.0 ** -149
MARGIN = 1.125
MUTANTS_ADAM = ('omb2_in_fp32', 'bias_correction_at_step_minus_1', 'bias_correction_at_step_plus_1', 'eps_inside_the_root',
                'decay_kinds_swapped', 'v_from_the_gradient_without_wd_p')
MUTANTS_ADAGRAD = ('eps_inside_the_root', 'sum_without_wd_p')


def _finish(b):
    return MARGIN * b + TINY


def _root_and_quotient(num, dnum, x, dx, div, eps, ss):
    """num / (sqrt(x) / div + eps) * ss with the errors dnum of num and dx of x -> (den, r, ds-chain error dw of ss * r)"""
    u = U32
    s = x.sqrt()
    ds = torch.minimum(dx / (s + (x - dx).clamp_min(0).sqrt()), dx.sqrt())
    ds = ds + 2 * u * (s + ds)
    q = s / div
    dq = ds / div + (3 * u * q if div != 1.0 else 0.0)
    den = q + eps
    dden = dq + u * eps + u * den
    den_lo = den - dden
    den_lo = torch.where(den_lo > 0, den_lo, torch.zeros_like(den_lo))
    r = num / den
    dr = dnum / den_lo + num.abs() * dden / (den * den_lo) + 2 * u * r.abs() + ETA
    return den, r, ss * (dr + 2 * u * r.abs()) + ETA


def adam_ref(kind, p, g, m, v, lr, b1, b2, eps, wd, step, e_in=None):
    """kind 0 AdamW, 1 Adam -> ((p', m', v'), (bp, bm, bv)), all float64; e_in = (e_p, e_m, e_v): errors the state already carries"""
    u = U32
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    e_p, e_m, e_v = e_in if e_in is not None else (0.0, 0.0, 0.0)
    omb1, omb2 = 1.0 - b1, 1.0 - b2
    if kind == 0:
        decay = 1.0 - lr * wd
        p1, g1 = p * decay, g
        dg = 0.0
        e_p1 = abs(decay) * e_p + ((2 * u * p1.abs() + ETA) if decay != 1.0 else 0.0)
    else:
        p1, g1 = p, g + wd * p
        dg = u * g1.abs() + 2 * u * abs(wd) * p.abs() + ETA + abs(wd) * e_p
        e_p1 = e_p
    m1 = m + (g1 - m) * omb1
    c = omb2 * g1 * g1
    v1 = v * b2 + c
    bm = b1 * e_m + u * m1.abs() + 3 * u * omb1 * (g1 - m).abs() + omb1 * dg + ETA
    bv = b2 * e_v + u * (v1 + 2 * b2 * v + 3 * c) + 2 * omb2 * g1.abs() * dg + omb2 * dg * dg + ETA * (2 + g1.abs())
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    ss = lr / bc1
    _, r, dw = _root_and_quotient(m1, bm, v1, bv, math.sqrt(bc2), eps, ss)
    p2 = p1 - ss * r
    bp = e_p1 + dw + u * p2.abs()
    return (p2, m1, v1), (_finish(bp), _finish(bm), _finish(bv))


def adagrad_ref(p, g, s, lr, eps, wd):
    """-> ((p', state_sum'), (bp, bs)), float64"""
    u = U32
    p, g, s = p.double(), g.double(), s.double()
    g1 = g + wd * p
    dg = u * g1.abs() + 2 * u * abs(wd) * p.abs() + ETA
    s1 = s + g1 * g1
    bs = u * (s1 + g1 * g1) + 2 * g1.abs() * dg + dg * dg + ETA
    _, r, dw = _root_and_quotient(g1, dg, s1, bs, 1.0, eps, lr)
    p2 = p - lr * r
    bp = dw + u * p2.abs()
    return (p2, s1), (_finish(bp), _finish(bs))


# ---- (c) fp32 restatement ------------------------------------------------------------------------------------------------------
def _np32(t):
    return (t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float32, copy=True)


def adam_f32(kind, p, g, m, v, lr, b1, b2, eps, wd, step, mutant=None):
    """adam_element of csrc/optim.hip in numpy float32 -> (p', m', v') float32 arrays"""
    f = np.float32
    assert mutant is None or mutant in MUTANTS_ADAM
    p, g, m, v = _np32(p), _np32(g), _np32(m), _np32(v)
    decoupled = kind == 0
    if mutant == 'decay_kinds_swapped':
        decoupled = not decoupled
    s_bc = step + {'bias_correction_at_step_minus_1': -1, 'bias_correction_at_step_plus_1': 1}.get(mutant, 0)
    bc1, bc2 = 1.0 - b1 ** s_bc, 1.0 - b2 ** s_bc
    with np.errstate(all='ignore'):
        step_size = f(np.float64(lr) / np.float64(bc1))
        bc2_sqrt = f(np.sqrt(np.float64(bc2)))
        decay, omb1, omb2, b2f, epsf, wdf = f(1.0 - lr * wd), f(1.0 - b1), f(1.0 - b2), f(b2), f(eps), f(wd)
        if mutant == 'omb2_in_fp32':
            omb2 = f(1.0) - f(b2)
        g_v = g
        if decoupled:
            p = p * decay
        else:
            t = wdf * p
            g = g + t
        if mutant != 'v_from_the_gradient_without_wd_p':
            g_v = g
        d = g - m
        t = d * omb1
        m = m + t
        a = v * b2f
        c = omb2 * g_v
        c = c * g_v
        v = a + c
        if mutant == 'eps_inside_the_root':
            s = np.sqrt(v + epsf)
            den = s / bc2_sqrt
        else:
            s = np.sqrt(v)
            q = s / bc2_sqrt
            den = q + epsf
        r = m / den
        w = step_size * r
        p = p - w
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def adagrad_f32(p, g, s, lr, eps, wd, mutant=None):
    """adagrad_kernel in numpy float32, no contraction -> (p', state_sum')"""
    f = np.float32
    assert mutant is None or mutant in MUTANTS_ADAGRAD
    p, g, s = _np32(p), _np32(g), _np32(s)
    lrf, epsf, wdf = f(lr), f(eps), f(wd)
    with np.errstate(all='ignore'):
        t = wdf * p
        ge = g + t
        g_s = g if mutant == 'sum_without_wd_p' else ge
        t = g_s * g_s
        s = s + t
        if mutant == 'eps_inside_the_root':
            den = np.sqrt(s + epsf)
        else:
            den = np.sqrt(s)
            den = den + epsf
        r = ge / den
        w = lrf * r
        p = p - w
    assert p.dtype == s.dtype == np.float32
    return p, s


# ---- the criterion ---------------------------------------------------------------------------------------------------------------
def check_bound(got, ref, bound, what):
    """|got - ref| <= bound on every element whose reference is finite (NaN in ``got`` fails there); elsewhere the class must agree:
    NaN with NaN, +-inf with the same inf. -> the largest err / bound"""
    got = torch.as_tensor(got).double()
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isnan(got[~fin]), torch.isnan(ref[~fin])) and bool((got[~fin] == ref[~fin])[~torch.isnan(ref[~fin])].all()), \
        f'{what}: a non-finite element is of another class than the float64 rule gives'
    err, bnd = (got[fin] - ref[fin]).abs(), bound[fin]
    bad = ~(err <= bnd)
    assert not bool(bad.any()), (f'{what}: derived bound exceeded at {int(bad.sum())} of {bad.numel()} elements, worst err '
                                 f'{float(err[bad].max()) if bool(torch.isfinite(err[bad]).any()) else float("nan"):.3e} at bound '
                                 f'{float(bnd[bad][0]):.3e}')
    return float((err / bnd).max()) if err.numel() else 0.0
