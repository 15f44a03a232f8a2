"""References for RecVAE's two row-wise kernels (csrc/recvae.hip: ``sbr_swish_ln_fwd`` / ``_bwd``, ``sbr_prior_kl_fwd`` / ``_bwd``;
``ops.SwishLayerNormFn``, ``ops.CompositePriorKLFn``) and for the model (recvae.py), and the cases their tests share. A plain module: numpy
and torch on the CPU, no fixtures, no GPU.

The definitions are those of RecVAE (Shenbin et al., WSDM 2020) as the authors' published code states them, AS REMEMBERED: that code
could not be fetched while this was written, so nothing here is checked against it (layer count, the LayerNorm eps of 0.1, the mixture
weights 3/20, 3/4, 1/10, the wide component's log-variance 10, gamma = 0.005 times the interaction count).

Three things:
  1. the float64 definitions in torch (``swish_ln64``, ``prior_kl64``, ``forward``), with gradients by autograd;
  2. a float32 restatement of the two ops in the kernels' order (``swish_ln32``, ``prior_kl32``): element j of a row on lane j % 64, a
     lane's elements in ascending order, the xor butterfly 32, 16, .. 1, no fused product-sums; the slab order of d gamma / d beta;
  3. the derived error bounds (``swish_ln_bound``, ``prior_kl_bound``).

The bounds are a running error analysis: every operation of the kernel is done once more in float64 on a pair (value, err), where err
bounds |computed fp32 value - value|. u = 2^-24. With |a^ - a| <= ea and |b^ - b| <= eb:
  a + b:  ea + eb + u (|a + b| + ea + eb)                    a * b:  t = |a| eb + |b| ea + ea eb;  t + u (|a b| + t)
  a / b:  t = (ea + |a / b| eb) / (|b| - eb);  t + u (|a / b| + t)             2^k a, -a, max: exact (max: between max(a - ea) and max(a + ea))
  sqrt(a): ea / (2 sqrt(a - ea)) + u sqrt(a)                 (correctly rounded, as is the division: hipcc's default)
  expf(a): exp(a + ea) - exp(a) + E_EXP exp(a + ea) + 2^-126      logf(a): log(a / (a - ea)) + E_LOG |log a|
  E(a), the correctly rounded exponential of an exact a:  u exp(a)
  a sum of n terms through at most k additions each:  sum of the terms' errs + gamma(k) (sum |term| + sum err),  gamma(k) = k u / (1 - k u)
A row sum of width W goes through ceil(W / 64) lane-local additions and 6 butterfly levels: k = ceil(W / 64) + 6. A column sum (d gamma,
d beta) goes through rps additions in a wave, 3 across the waves (rps = max(1, ceil(B / 4096)) rows per wave), then the slabs are added
in double and rounded once: k = rps + 4. The operation count per output is therefore what the kernel text does, no more: the value
halves of the pairs ARE the closed-form float64 forward and backward formulas, and tests/test_recvae_cpu.py checks them against autograd.
E_EXP and E_LOG are those of tests/multvae_ref.py (twice the measured errors of the device's expf and logf)."""
import numpy as np
import scipy.sparse as sp
import torch

U = 2.0 ** -24
E_EXP = 2.0 * 2.0 ** -23
E_LOG = 4.6 * 2.0 ** -23
TINY = 2.0 ** -126
LOG2PI = float(np.log(2 * np.pi))
LOGW = (float(np.log(3 / 20)), float(np.log(3 / 4)), float(np.log(1 / 10)))
V2 = 10.0
LN_EPS = 0.1
MAX_W = 1024
F32 = np.float32

H_SIZES = [1, 2, 63, 64, 65, 600, 1024]
L_SIZES = [1, 63, 64, 65, 200, 1024]
BATCHES = [1, 3, 4, 5, 67]


def gamma_k(k):
    return k * U / (1 - k * U)


def rows_per_wave(B):
    return max(1, -(-B // 4096))


def slabs(B):
    return 0 if B <= 0 else -(-B // (4 * rows_per_wave(B)))


# ---- 1. the float64 definitions (torch, any dtype) ------------------------------------------------------------------------------------------
def swish_ln64(a, r_in, gamma, beta, eps=LN_EPS):
    """-> (h, r_out): h = LN(swish(a + r_in)), r_out = r_in + h (r_in None: s = a, r_out = h)"""
    s = a if r_in is None else a + r_in
    y = s * torch.sigmoid(s)
    d = y - y.mean(1, keepdim=True)
    h = d / torch.sqrt((d * d).mean(1, keepdim=True) + eps) * gamma + beta
    return h, (h if r_in is None else r_in + h)


def log_normal(z, m, v):
    return -0.5 * (v + LOG2PI + (z - m) ** 2 / torch.exp(v))


def prior_kl64(mu, logvar, eps, mu_old, logvar_old, weight):
    """-> (z, row_kl): z = mu + eps exp(logvar / 2), row_kl = weight * sum_j (log N(z; mu, logvar) - log p(z))"""
    z = mu + eps * torch.exp(0.5 * logvar)
    zero = torch.zeros_like(z)
    comps = torch.stack([LOGW[0] + log_normal(z, zero, zero), LOGW[1] + log_normal(z, mu_old, logvar_old),
                         LOGW[2] + log_normal(z, zero, zero + V2)])
    return z, weight * (log_normal(z, mu, logvar) - torch.logsumexp(comps, 0)).sum(1)


# ---- 2. the float32 restatement in the kernels' order -----------------------------------------------------------------------------------------
def _exp32(x):
    """an expf: the float64 exponential rounded once"""
    with np.errstate(over='ignore', under='ignore'):
        return np.exp(x.astype(np.float64)).astype(F32)


def _log32(x):
    return np.log(x.astype(np.float64)).astype(F32)


def _row_sum32(t):
    """t [B, W] float32 -> [B]: lane j % 64 adds its elements in ascending order from +0, then the butterfly 32, 16, .. 1"""
    B, W = t.shape
    K = -(-W // 64)
    pad = np.zeros((B, 64 * K), dtype=F32)
    pad[:, :W] = t
    lanes = np.zeros((B, 64), dtype=F32)
    for k in range(K):
        valid = (np.arange(64) + 64 * k) < W
        lanes = np.where(valid, lanes + pad[:, 64 * k:64 * k + 64], lanes).astype(F32)
    o = 32
    while o:
        lanes = (lanes + lanes[:, np.arange(64) ^ o]).astype(F32)
        o >>= 1
    return lanes[:, 0]


def _col_sum32(t):
    """t [B, W] float32 -> [W]: the slab partials (a wave's rows in ascending order, then the four waves), the slabs in double"""
    B, W = t.shape
    rps = rows_per_wave(B)
    total = np.zeros(W, dtype=np.float64)
    for sl in range(slabs(B)):
        first = sl * 4 * rps
        waves = []
        for q in range(4):
            acc = np.zeros(W, dtype=F32)
            for i in range(rps):
                b = first + q + 4 * i
                if b < B:
                    acc = (acc + t[b]).astype(F32)
            waves.append(acc)
        part = waves[0]
        for q in range(1, 4):
            part = (part + waves[q]).astype(F32)
        total += part.astype(np.float64)
    return total.astype(F32)


def _sigmoid32(s):
    one = F32(1)
    return (one / (one + _exp32(-s))).astype(F32)


def swish_ln32(a, r_in, gamma, beta, eps=LN_EPS, dh=None, dr_out=None):
    """float32 arrays -> dict(s, h, r_out, mean, rstd) and, with dh or dr_out, (da, dr_in, dgamma, dbeta), in the kernels' order"""
    a, gamma, beta = a.astype(F32), gamma.astype(F32), beta.astype(F32)
    fh = F32(a.shape[1])
    s = a if r_in is None else (a + r_in.astype(F32)).astype(F32)
    sig = _sigmoid32(s)
    y = (s * sig).astype(F32)
    mean = (_row_sum32(y) / fh).astype(F32)
    d = (y - mean[:, None]).astype(F32)
    rstd = (F32(1) / np.sqrt((_row_sum32((d * d).astype(F32)) / fh + F32(eps)).astype(F32))).astype(F32)
    h = (((d * rstd[:, None]).astype(F32) * gamma).astype(F32) + beta).astype(F32)
    out = dict(s=s, h=h, mean=mean, rstd=rstd, r_out=h if r_in is None else (r_in.astype(F32) + h).astype(F32))
    if dh is None and dr_out is None:
        return out
    g = dh.astype(F32) if dr_out is None else (dr_out.astype(F32) if dh is None else (dh.astype(F32) + dr_out.astype(F32)).astype(F32))
    xh = ((y - mean[:, None]).astype(F32) * rstd[:, None]).astype(F32)
    dsw = (sig + (y * (F32(1) - sig).astype(F32)).astype(F32)).astype(F32)
    gg = (g * gamma).astype(F32)
    c1 = (_row_sum32(gg) / fh).astype(F32)
    c2 = (_row_sum32((gg * xh).astype(F32)) / fh).astype(F32)
    inner = ((gg - c1[:, None]).astype(F32) - (xh * c2[:, None]).astype(F32)).astype(F32)
    ds = ((rstd[:, None] * inner).astype(F32) * dsw).astype(F32)
    out.update(da=ds, dr_in=ds if dr_out is None else (ds + dr_out.astype(F32)).astype(F32), dgamma=_col_sum32((g * xh).astype(F32)),
               dbeta=_col_sum32(g))
    return out


def z32(mu, logvar, eps):
    """the float32 z = mu + eps * E(0.5 * logvar), E the correctly rounded exponential: what the kernel's z equals bit for bit"""
    return (mu.astype(F32) + (eps.astype(F32) * _exp32((F32(0.5) * logvar.astype(F32)).astype(F32))).astype(F32)).astype(F32)


def _mix32(z, mo, lvo):
    half = F32(0.5)
    with np.errstate(over='ignore'):
        zz = (z * z).astype(F32)
        d = (z - mo).astype(F32)
        l0 = (F32(LOGW[0]) - (half * (F32(LOG2PI) + zz).astype(F32)).astype(F32)).astype(F32)
        q1 = ((d * d).astype(F32) / _exp32(lvo)).astype(F32)
        l1 = (F32(LOGW[1]) - (half * ((lvo + F32(LOG2PI)).astype(F32) + q1).astype(F32)).astype(F32)).astype(F32)
        q2 = (zz / F32(np.exp(V2))).astype(F32)
        l2 = (F32(LOGW[2]) - (half * ((F32(V2) + F32(LOG2PI)).astype(F32) + q2).astype(F32)).astype(F32)).astype(F32)
    mx = np.maximum(np.maximum(l0, l1), l2)
    e = [_exp32((l - mx).astype(F32)) for l in (l0, l1, l2)]
    se = ((e[0] + e[1]).astype(F32) + e[2]).astype(F32)
    return mx, e, se


def prior_kl32(mu, logvar, eps, mu_old, logvar_old, weight, dz=None, upstream=None, scale=0.0):
    """float32 arrays -> dict(z, row_kl) and, with ``scale`` (1 / B) or dz, (dmu, dlogvar), in the kernels' order"""
    mu, logvar, eps, mo, lvo, weight = (t.astype(F32) for t in (mu, logvar, eps, mu_old, logvar_old, weight))
    half = F32(0.5)
    z = z32(mu, logvar, eps)
    lq = (-half * ((logvar + F32(LOG2PI)).astype(F32) + (eps * eps).astype(F32)).astype(F32)).astype(F32)
    mx, e, se = _mix32(z, mo, lvo)
    lp = (mx + _log32(se)).astype(F32)
    out = dict(z=z, row_kl=(weight * _row_sum32((lq - lp).astype(F32))).astype(F32))
    if dz is None and upstream is None and not scale:
        return out
    up = F32(scale) if upstream is None else (F32(upstream) * F32(scale)).astype(F32)
    c = (up * weight).astype(F32)[:, None]
    with np.errstate(over='ignore', invalid='ignore'):
        t1 = (e[1] * ((z - mo).astype(F32) / _exp32(lvo)).astype(F32)).astype(F32)
        num = (((e[0] * z).astype(F32) + t1).astype(F32) + (e[2] * (z / F32(np.exp(V2))).astype(F32)).astype(F32)).astype(F32)
    dlp = -(num / se).astype(F32)
    t = -(c * dlp).astype(F32)
    if dz is not None:
        t = (dz.astype(F32) + t).astype(F32)
    sd = _exp32((half * logvar).astype(F32))
    out.update(dmu=t, dlogvar=((t * (half * (eps * sd).astype(F32)).astype(F32)).astype(F32) - (half * c).astype(F32)).astype(F32))
    return out


# ---- 3. the derived bounds: running error analysis ---------------------------------------------------------------------------------------------
class E:
    """(value, err): err bounds |the kernel's fp32 value - value|; every method is one rounded fp32 operation unless it says exact"""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape)

    def __add__(self, o):
        o = _E(o)
        v = self.v + o.v
        t = self.e + o.e
        return E(v, t + U * (np.abs(v) + t))

    def __sub__(self, o):
        return self + (-_E(o))

    def __neg__(self):
        return E(-self.v, self.e)

    def __mul__(self, o):
        o = _E(o)
        v = self.v * o.v
        t = np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e
        return E(v, t + U * (np.abs(v) + t))

    def __truediv__(self, o):
        o = _E(o)
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            v = self.v / o.v
            room = np.abs(o.v) - o.e
            t = np.where(room > 0, (self.e + np.abs(v) * o.e) / np.where(room > 0, room, 1.0), np.inf)
        return E(v, t + U * (np.abs(v) + t))

    def half(self):
        return E(0.5 * self.v, 0.5 * self.e)                               # exact

    def exp(self, rel=E_EXP):
        with np.errstate(over='ignore', under='ignore', invalid='ignore'):
            v, hi = np.exp(self.v), np.exp(self.v + self.e)
            return E(v, (hi - v) + rel * hi + TINY)

    def log(self):
        with np.errstate(divide='ignore', invalid='ignore'):
            room = self.v - self.e
            t = np.where(room > 0, np.log(self.v / np.where(room > 0, room, 1.0)), np.inf)
            return E(np.log(self.v), t + E_LOG * np.abs(np.log(self.v)))

    def sqrt(self):
        room = self.v - self.e
        assert (room > 0).all()
        return E(np.sqrt(self.v), self.e / (2 * np.sqrt(room)) + U * np.sqrt(self.v))

    def row_sum(self):
        k = -(-self.v.shape[1] // 64) + 6
        t = self.e.sum(1)
        return E(self.v.sum(1), t + gamma_k(k) * (np.abs(self.v).sum(1) + t))

    def col_sum(self):
        k = rows_per_wave(self.v.shape[0]) + 4
        t = self.e.sum(0)
        return E(self.v.sum(0), t + gamma_k(k) * (np.abs(self.v).sum(0) + t))

    def col(self):
        return E(self.v[:, None], self.e[:, None])


def _E(x):
    return x if isinstance(x, E) else E(x)


def emax(*xs):
    """exact; the computed maximum lies between max(x - err) and max(x + err)"""
    v = np.maximum.reduce([x.v for x in xs])
    hi, lo = np.maximum.reduce([x.v + x.e for x in xs]), np.maximum.reduce([x.v - x.e for x in xs])
    return E(v, np.maximum(hi - v, v - lo))


def _sigmoid_e(s):
    return E(1.0) / (E(1.0) + (-s).exp())


def swish_ln_bound(a, r_in, gamma, beta, eps=LN_EPS, dh=None, dr_out=None):
    """-> {name: E}: the float64 closed forms (``.v``) and the bounds (``.e``) of everything the two entries write, the backward pass
    taking s, mean and rstd as the forward kernel leaves them (their errors are carried on)"""
    fh = float(a.shape[1])
    s = E(a) if r_in is None else E(a) + E(r_in)
    sig = _sigmoid_e(s)
    y = s * sig
    mean = y.row_sum() / fh
    d = y - mean.col()
    rstd = E(1.0) / ((d * d).row_sum() / fh + float(F32(eps))).sqrt()
    h = d * rstd.col() * E(gamma) + E(beta)
    out = dict(s=s, h=h, mean=mean, rstd=rstd, r_out=h if r_in is None else E(r_in) + h)
    if dh is None and dr_out is None:
        return out
    g = E(dh) if dr_out is None else (E(dr_out) if dh is None else E(dh) + E(dr_out))
    xh = (y - mean.col()) * rstd.col()
    dsw = sig + y * (E(1.0) - sig)
    gg = g * E(gamma)
    c1, c2 = gg.row_sum() / fh, (gg * xh).row_sum() / fh
    ds = rstd.col() * ((gg - c1.col()) - xh * c2.col()) * dsw
    out.update(da=ds, dr_in=ds if dr_out is None else ds + E(dr_out), dgamma=(g * xh).col_sum(), dbeta=g.col_sum())
    for k in ('dgamma', 'dbeta'):                                          # the double sum of the slabs is rounded once
        out[k] = E(out[k].v, out[k].e + U * (np.abs(out[k].v) + out[k].e))
    return out


def _const(x, e, scale):
    """x with the rounding of an fp32 constant of magnitude ``scale`` that entered it added to its err"""
    return E(x.v, x.e + U * scale)


def _mix_e(z, mo, lvo):
    """the constants LOG2PI, log w_c and exp(10) are fp32 in the kernel: each adds u times its share of l_c to the err of l_c"""
    zz = z * z
    d = z - mo
    l0 = _const(E(LOGW[0]) - (E(LOG2PI) + zz).half(), 0, abs(LOGW[0]) + LOG2PI)
    l1 = _const(E(LOGW[1]) - (lvo + LOG2PI + d * d / lvo.exp()).half(), 0, abs(LOGW[1]) + LOG2PI)
    l2 = E(LOGW[2]) - (E(V2) + LOG2PI + zz / float(np.exp(V2))).half()
    l2 = _const(l2, 0, abs(LOGW[2]) + LOG2PI + zz.v / np.exp(V2))
    mx = emax(l0, l1, l2)
    e = [(l - mx).exp() for l in (l0, l1, l2)]
    return mx, e, e[0] + e[1] + e[2]


def prior_kl_bound(mu, logvar, eps, mu_old, logvar_old, weight, dz=None, upstream=None, scale=0.0):
    """-> {name: E} for z, row_kl and (with dz or scale) dmu, dlogvar; ``.v`` are the closed forms in float64"""
    mu, lv, ep, mo, lvo = E(mu), E(logvar), E(eps), E(mu_old), E(logvar_old)
    sd = lv.half().exp(rel=U)
    z = mu + ep * sd
    lq = _const(-((lv + LOG2PI + ep * ep).half()), 0, LOG2PI)
    mx, e, se = _mix_e(z, mo, lvo)
    out = dict(z=z, row_kl=E(weight) * (lq - (mx + se.log())).row_sum())
    if dz is None and upstream is None and not scale:
        return out
    up = E(float(F32(scale))) if upstream is None else E(float(F32(upstream))) * E(float(F32(scale)))
    c = (up * E(weight)).col()
    far = _const(z / float(np.exp(V2)), 0, np.abs(z.v) / np.exp(V2))
    num = e[0] * z + e[1] * ((z - mo) / lvo.exp()) + e[2] * far
    t = c * (num / se)                                                     # -(c * dlp) = c * num / se: the two negations are exact
    if dz is not None:
        t = E(dz) + t
    out.update(dmu=t, dlogvar=t * (ep * sd).half() - c.half())
    return out


def ratio(got, ref: E):
    """the largest |got - value| / err; an err of 0 admits no error; inf or NaN anywhere fails"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref.v)
    assert np.isfinite(err).all() and not np.isnan(ref.e).any()
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(ref.e > 0, err / ref.e, np.where(err == 0, 0.0, np.inf))
    return float(q.max()) if q.size else 0.0


# ---- the cases the CPU and GPU tests share --------------------------------------------------------------------------------------------------
def swish_ln_case(B, H, seed, with_sum=True):
    """float32 operands. Row b % 5 == 1 (when B > 1) has a mean of about 1e3 with unit spread: a one-pass variance fails there; row
    b % 5 == 2 is exactly constant (rstd = 1 / sqrt(eps), h = beta). gamma and beta are random, not (1, 0)."""
    rng = np.random.default_rng(1000 * H + 10 * B + seed)
    a = (2 * rng.standard_normal((B, H))).astype(F32)
    r = rng.standard_normal((B, H)).astype(F32) if with_sum else None
    for b in range(B):
        if b % 5 == 1:
            a[b] = (1000 + rng.standard_normal(H)).astype(F32)
            if r is not None:
                r[b] = 0
        if b % 5 == 2:
            a[b] = F32(0.75)
            if r is not None:
                r[b] = F32(-0.25)
    gamma = (1 + 0.5 * rng.standard_normal(H)).astype(F32)
    beta = rng.standard_normal(H).astype(F32)
    dh, dr = rng.standard_normal((B, H)).astype(F32), rng.standard_normal((B, H)).astype(F32)
    return a, r, gamma, beta, dh, dr


def prior_kl_case(B, L, seed):
    """float32 operands: logvar_old in {-20, 0, 10} per element, |z| up to 50 (every third row sits far from every component), weight
    with zeros in it"""
    rng = np.random.default_rng(2000 * L + 10 * B + seed)
    mu = rng.standard_normal((B, L))
    mu[::3] *= 15
    mu = np.clip(mu, -45, 45).astype(F32)
    logvar = rng.uniform(-4, 2, (B, L)).astype(F32)
    eps = np.clip(rng.standard_normal((B, L)), -1.8, 1.8).astype(F32)              # |eps| exp(1) < 5: |z| < 50
    mu_old = rng.standard_normal((B, L)).astype(F32)
    near = rng.random((B, L)) < 0.3                                              # some z within reach of the narrow component
    mu_old = np.where(near, mu + F32(1e-4) * mu_old, mu_old).astype(F32)
    logvar_old = rng.choice(np.array([-20, 0, 10], dtype=F32), size=(B, L))
    weight = (rng.uniform(0.05, 2, B) * (rng.random(B) > 0.25)).astype(F32)
    if B > 1:
        weight[B // 2] = 0
    dz = rng.standard_normal((B, L)).astype(F32)
    return mu, logvar, eps, mu_old, logvar_old, weight, dz


def t64(x):
    return None if x is None else torch.from_numpy(np.asarray(x, dtype=np.float64))


def swish_ln_autograd(a, r, gamma, beta, dh, dr_out, eps=LN_EPS):
    """float64 autograd of the definition -> dict(h, r_out, da, dr_in, dgamma, dbeta) as numpy"""
    A, G, Bt = t64(a).requires_grad_(), t64(gamma).requires_grad_(), t64(beta).requires_grad_()
    R = None if r is None else t64(r).requires_grad_()
    h, ro = swish_ln64(A, R, G, Bt, float(F32(eps)))
    obj = 0
    if dh is not None:
        obj = obj + (h * t64(dh)).sum()
    if dr_out is not None:
        obj = obj + (ro * t64(dr_out)).sum()
    obj.backward()
    return dict(h=h.detach().numpy(), r_out=ro.detach().numpy(), da=A.grad.numpy(), dr_in=None if R is None else R.grad.numpy(),
                dgamma=G.grad.numpy(), dbeta=Bt.grad.numpy())


def prior_kl_autograd(mu, logvar, eps, mu_old, logvar_old, weight, dz, upstream, scale):
    M, Lv = t64(mu).requires_grad_(), t64(logvar).requires_grad_()
    z, row = prior_kl64(M, Lv, t64(eps), t64(mu_old), t64(logvar_old), t64(weight))
    obj = float(F32(upstream)) * float(F32(scale)) * row.sum()
    if dz is not None:
        obj = obj + (z * t64(dz)).sum()
    obj.backward()
    return dict(z=z.detach().numpy(), row_kl=row.detach().numpy(), dmu=M.grad.numpy(), dlogvar=Lv.grad.numpy())


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------
N_LAYERS = 5
ENCODER_PARAMS = tuple(f'{kind}{k}' for k in range(1, N_LAYERS + 1) for kind in ('fc_w', 'fc_b', 'ln_w', 'ln_b')) + \
    ('mu_w', 'mu_b', 'logvar_w', 'logvar_b')
DECODER_PARAMS = ('dec_w', 'dec_b')
PARAMS = ENCODER_PARAMS + DECODER_PARAMS
N_USERS, N_ITEMS, N_BLOCKS = 48, 40, 4
SETTINGS = dict(hidden=32, latent=8, batch_size=16, lr=5e-3, dropout=0.5, gamma=0.005)


def init_params(n_items, hidden, latent, seed, dtype=torch.float64):
    """random parameters under the package's names, every one of a size that matters (LayerNorm weights and biases not (1, 0)), all
    fp32-representable"""
    g = torch.Generator().manual_seed(int(seed))
    p = {}
    for k in range(1, N_LAYERS + 1):
        inp = n_items if k == 1 else hidden
        p[f'fc_w{k}'] = torch.randn(hidden, inp, generator=g) * (4.0 / (hidden + inp)) ** 0.5
        p[f'fc_b{k}'] = torch.randn(hidden, generator=g) * 0.1
        p[f'ln_w{k}'] = 1 + 0.3 * torch.randn(hidden, generator=g)
        p[f'ln_b{k}'] = 0.2 * torch.randn(hidden, generator=g)
    for name in ('mu', 'logvar'):
        p[name + '_w'] = torch.randn(latent, hidden, generator=g) * (2.0 / (hidden + latent)) ** 0.5
        p[name + '_b'] = torch.randn(latent, generator=g) * 0.1
    p['dec_w'] = torch.randn(n_items, latent, generator=g) * (8.0 / (n_items + latent)) ** 0.5
    p['dec_b'] = torch.randn(n_items, generator=g) * 0.1
    return {k: v.float().to(dtype).requires_grad_() for k, v in p.items()}


def encode(p, xn):
    """xn [B, I]: the normalised (and dropped-out) rows -> (mu, logvar)"""
    h, r = swish_ln64(xn @ p['fc_w1'].t() + p['fc_b1'], None, p['ln_w1'], p['ln_b1'], LN_EPS)
    for k in range(2, N_LAYERS + 1):
        h, r = swish_ln64(h @ p[f'fc_w{k}'].t() + p[f'fc_b{k}'], r, p[f'ln_w{k}'], p[f'ln_b{k}'], LN_EPS)
    return h @ p['mu_w'].t() + p['mu_b'], h @ p['logvar_w'].t() + p['logvar_b']


def forward(p, old, x, eps, gamma=0.005, beta=None, keep=None, dropout=0.0):
    """The model in torch in the dtype of the parameters ``p``; ``old``: the old encoder's parameters (no gradient). x [B, I]: the 0/1 rows.
    -> (loss, nll, kld, logits, mu)"""
    dt = p['fc_w1'].dtype
    x = x.to(dt)
    xn = x / x.pow(2).sum(1, keepdim=True).sqrt().clamp(min=1e-8)
    xd = xn if keep is None else xn * keep.to(dt) / (1.0 - dropout)
    mu, logvar = encode(p, xd)
    with torch.no_grad():
        mu_old, logvar_old = encode(old, xn)
    n = x.sum(1)
    weight = gamma * n if gamma else torch.full_like(n, beta)
    z, row_kl = prior_kl64(mu, logvar, eps.to(dt), mu_old, logvar_old, weight)
    logits = z @ p['dec_w'].t() + p['dec_b']
    row = n * torch.logsumexp(logits, 1) - (logits * x).sum(1)
    nll = torch.where(n > 0, row, torch.zeros_like(row)).mean()
    kld = row_kl.mean()
    return nll + kld, nll, kld, logits, mu


def planted_world(seed=0):
    """48 users x 40 items in 4 blocks; a user has 5 to 8 items of their block -> train csr (sorted indices)"""
    rng = np.random.default_rng(3000 + seed)
    ub, ib = N_USERS // N_BLOCKS, N_ITEMS // N_BLOCKS
    rows, cols = [], []
    for u in range(N_USERS):
        items = (u // ub) * ib + rng.choice(ib, size=int(rng.integers(5, 9)), replace=False)
        rows += [u] * len(items)
        cols += list(items)
    m = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(N_USERS, N_ITEMS))
    m.sort_indices()
    return m


def model_errors(seed=3):
    """One loss and all parameter gradients of the model on the planted world in float64 and in float32 torch on the CPU, the same
    weights, the same eps, dropout 0, the old encoder a perturbed copy -> (out64, grads64, out32, grads32, p64, old64, x, eps)"""
    x = torch.from_numpy(np.asarray(planted_world(0).todense(), dtype=np.float64))
    p64 = init_params(N_ITEMS, SETTINGS['hidden'], SETTINGS['latent'], seed)
    old64 = {k: v.detach().clone() for k, v in init_params(N_ITEMS, SETTINGS['hidden'], SETTINGS['latent'], seed + 1).items() if k in ENCODER_PARAMS}
    eps = torch.randn(N_USERS, SETTINGS['latent'], generator=torch.Generator().manual_seed(seed)).double()
    out64 = forward(p64, old64, x, eps)
    out64[0].backward()
    p32 = {k: v.detach().float().requires_grad_() for k, v in p64.items()}
    old32 = {k: v.float() for k, v in old64.items()}
    out32 = forward(p32, old32, x, eps)
    out32[0].backward()
    return out64, {k: p64[k].grad for k in PARAMS}, out32, {k: p32[k].grad for k in PARAMS}, p64, old64, x, eps
