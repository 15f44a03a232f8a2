"""Float64 references, derived error bounds and exact operand families for the dense GEMM family (csrc/gemm_f32.hip, gemm_ring_f32.hip,
gemm_wres_f32.hip, gemm_split_f32.hip, gemm_split_wide_f32.hip, gemm_split_tn_f32.hip and the slab reducers). A plain module: no
fixtures, no pytest hooks, no GPU. tests/test_gemm_refs_cpu.py shows on the CPU that the criteria below accept a right kernel and
reject a wrong one; tests/test_hip_gemm.py applies them to the kernels.

References (the definitions of include/sibrar_hip.h, evaluated in float64 on the operands' own storage: flat array + leading
dimension + optional int32 row map, exactly what the C entry takes):
    NT  C[ci(m), n] = act(sum_k A[ai(m), k] B[n, k] + bias[n])
    NN  C[m, n]     = sum_k A[ai(m), k] B[k, n]
    TN  C[m, n]     = sum_k A[ak(k), m] B[bk(k), n]
each returns (out, pre, S): the result, the pre-activation and S = sum_k |a_k| |b_k| (+ |bias|) per output element.

Bounds — derived, never fitted. u = 2^-24 is the unit roundoff of fp32 (hip_testutil.U32), gamma(m) = m u / (1 - m u).

  fp32-pipe kernels (sbr_gemm_f32 in all modes, the ring kernel, sbr_gemm_wres_f32, sbr_gemm_nt_splitk_f32, sbr_gemm_tn_f32 on the
  ring / tile kernels). v_mfma_f32_32x32x2_f32 is an fmaf chain, but the bound does not rely on the fusion: each of the K products
  rounds once, and a sum of K terms in ANY order (the chain of one workgroup, split-K slabs added by the reducer, float atomics in
  arrival order) puts every term through at most K - 1 additions, each rounding once. The bias add is one more addition. To first
  order |err| <= (K + 2) u S (one rounding in hand); asserted in the gamma form:
        BOUND_F32 = gamma(K + 2) S.

  bf16-split kernels (sbr_gemm_split_f32, sbr_gemm_split_proj_f32, sbr_gemm_split_wide_f32, the split TN kernel behind
  sbr_gemm_tn_f32). gemm_split_common.h: sp_split2 splits x = x0 + x1 + x2 with x0 = bf16_rne(x), x1 = bf16_rne(x - x0),
  x2 = bf16_rne(x - x0 - x1). The conversion (__builtin_convertvector to __bf16) ROUNDS TO NEAREST EVEN, it does not truncate, so
        |x - x0| <= 2^-9 ulp-wise = 2^-8 |x| at most,  |x1| <= 2^-8 |x|,  |x2| <= 2^-16 |x|,  |x0| <= (1 + 2^-8) |x|,
  both subtractions are exact in fp32 and the last remainder has at most 8 significant bits (x2 exact). Each 8 x 8-bit partial
  product is exact in fp32. The kernels keep the six terms (i, j), i + j <= 2, and drop (1,2), (2,1), (2,2):
        |dropped| <= (2 * 2^-24 + 2^-32) |a b| = (2 + 2^-8) u |a b|         (a truncating split would give 4 u: |x1| < 2^-7 |x|)
  The kept terms of one product sum in absolute value to at most
        (1 + 2^-8)^2 + 2 (1 + 2^-8) 2^-8 + 2 (1 + 2^-8) 2^-16 + 2^-16 = 1 + 2^-6 + 3 * 2^-15 + 2^-23  <  F = 1 + 2^-6 + 2^-13
  times |a b|. (The issue's starting figure 1 + 2^-6 forgets the squares of the 2^-8 terms; F is the corrected factor.) The 6K kept
  terms and the bias are 6K + 1 terms added in some order: at most 6K roundings per term. To first order
  (6K + 2 + 2^-8) u F S; asserted with the head-room of the truncating split's constant:
        BOUND_SPLIT = gamma(6K + 8) F S.
  The bf16 MFMA adds its 16 products and the accumulator inside the instruction; the bound allows every one of those additions a
  full rounding, which no rounding-to-nearest adder exceeds.

  Epilogues. relu is 1-Lipschitz and exact. tanh, sigmoid and selu propagate the pre-activation bound with the activation's
  Lipschitz constant (hip_testutil.LIP) and add their own evaluation error, EXP_ULP (2 ulp) per transcendental call, exactly as
  test_hip_tail.bound_bn_fwd does: tanh EXP_ULP |y|; sigmoid (EXP_ULP + 2 u) |y| (expf, one addition, one division); selu u |y| for
  pre > 0, else scale alpha (EXP_ULP e^pre + 3 u |e^pre - 1|).

Exact operand families. At K = 128 the worst-case bound is about 2^-14 S: it cannot see a dropped third-plane term (2^-17). So
every random case has companions whose float64 result is exactly representable in fp32 and must be matched AS VALUES (torch.equal;
-0 == +0):
  ints              dense operands from {-3..3}, integer bias in {-8..8}: every partial sum is an integer of magnitude at most
                    9 K + 8 < 2^24 up to K = 600,000 (asserted in test_gemm_refs_cpu.py), so every summation order is exact, and
                    every value lies in the first bf16 plane. Pins indexing, k coverage, tile edges, gathers and the scatter.
  onehot_full       one operand has one non-zero per reduction (a signed power of two), the other carries 24-bit significands
                    1.0xxx...x1 (leading fraction bit 0, last bit 1): the output is a scaled copy of one element. The leading
                    fraction bit is kept 0 so that bf16_rne(x) never carries into the next binade: then every partial sum of the
                    planes x0, x1, x2 is representable and the three terms may be added in any order. Role 'a' (A one-hot) pins the
                    (0, j) plane terms, role 'b' the (j, 0) terms.
  onehot_two_plane  both operands are +-2^e (1 + 2^-10) (planes 2^e, 2^(e-10), 0), one of them one-hot: the single product
                    2^(e+f) (1 + 2^-9 + 2^-20) has 21 significant bits — exact in fp32 in any order of its four terms — and its
                    last bit is the (1,1) term.
"""
import numpy as np
import torch

from hip_testutil import EXP_ULP, LIP, SELU_AF, SELU_SF, U32, ref_act

F_SPLIT = 1.0 + 2.0 ** -6 + 2.0 ** -13
INT_MAX_ABS, INT_BIAS_MAX = 3, 8
K_MAX_GPU = 600_000                          # the longest reduction of tests/test_hip_gemm.py
FAMILIES_EXACT = ('ints', 'onehot_full_a', 'onehot_full_b', 'onehot_two_plane_a', 'onehot_two_plane_b')


def gamma(m):
    assert m * U32 < 0.5
    return m * U32 / (1.0 - m * U32)


# ---- storage access ----------------------------------------------------------------------------------------------------------
def mat(flat, ld, rows, cols):
    """[rows, cols] float64 copy of the row-major matrix with row stride ld that starts at flat[0]"""
    return torch.as_strided(flat, (rows, cols), (ld, 1)).double()


def _rows_of(flat, ld, idx, n, cols, n_table=None):
    if idx is None:
        return mat(flat, ld, n, cols)
    idx = torch.as_tensor(np.asarray(idx), dtype=torch.long)
    assert idx.numel() == n
    return mat(flat, ld, int(idx.max()) + 1 if n_table is None else n_table, cols)[idx]


def _finish(pre, S, act):
    return ref_act(pre, act), pre, S


def ref_nt(A, lda, a_idx, B, ldb, bias, M, N, K, act=0):
    a, b = _rows_of(A, lda, a_idx, M, K), mat(B, ldb, N, K)
    pre, S = a @ b.t(), a.abs() @ b.abs().t()
    if bias is not None:
        pre, S = pre + bias.double()[None, :N], S + bias.double().abs()[None, :N]
    return _finish(pre, S, act)


def ref_nn(A, lda, a_idx, B, ldb, M, N, K, b_idx=None):
    """b_idx: sbr_gemm_f32 mode 1 also takes a map of B's k rows (C[m, n] = sum_k A[ai(m), k] B[bk(k), n])"""
    a, b = _rows_of(A, lda, a_idx, M, K), _rows_of(B, ldb, b_idx, K, N)
    return _finish(a @ b, a.abs() @ b.abs(), 0)


def ref_tn(A, lda, a_idx, B, ldb, b_idx, M, N, K, bias=None):
    """bias: sbr_gemm_f32 mode 2 adds bias[n] once to what it accumulates"""
    a, b = _rows_of(A, lda, a_idx, K, M), _rows_of(B, ldb, b_idx, K, N)
    pre, S = a.t() @ b, a.abs().t() @ b.abs()
    if bias is not None:
        pre, S = pre + bias.double()[None, :N], S + bias.double().abs()[None, :N]
    return _finish(pre, S, 0)


# ---- bounds --------------------------------------------------------------------------------------------------------------------
def _act_bound(pre_bound, out, pre, act):
    y = out.abs()
    own = {0: 0.0, 1: 0.0, 2: EXP_ULP * y, 3: (EXP_ULP + 2 * U32) * y,
           4: torch.where(pre > 0, U32 * y, SELU_SF * SELU_AF * (EXP_ULP * torch.exp(pre.clamp_max(0)) + 3 * U32 * torch.expm1(pre.clamp_max(0)).abs()))}[act]
    return LIP[act] * pre_bound + own


def bound_f32(S, K, out=None, pre=None, act=0):
    b = gamma(K + 2) * S
    return b if act == 0 else _act_bound(b, out, pre, act)


def bound_split(S, K, out=None, pre=None, act=0):
    b = gamma(6 * K + 8) * F_SPLIT * S
    return b if act == 0 else _act_bound(b, out, pre, act)


# ---- operands ------------------------------------------------------------------------------------------------------------------
def _g(seed):
    return torch.Generator().manual_seed(seed)


def _sign(shape, g):
    return torch.randint(0, 2, shape, generator=g).float() * 2 - 1


def _pow2(shape, g, lo=-4, hi=4):
    return _sign(shape, g) * torch.exp2(torch.randint(lo, hi + 1, shape, generator=g).float())


def gen_rand6(shape, seed):
    """signed magnitudes spread log-uniformly over six decades, 1e-3 .. 1e3"""
    g = _g(seed)
    return (_sign(shape, g) * torch.pow(10.0, torch.rand(shape, generator=g, dtype=torch.float64) * 6 - 3)).float()


def gen_ints(shape, seed):
    return torch.randint(-INT_MAX_ABS, INT_MAX_ABS + 1, shape, generator=_g(seed)).float()


def gen_int_bias(n, seed):
    return torch.randint(-INT_BIAS_MAX, INT_BIAS_MAX + 1, (n,), generator=_g(seed)).float()


def gen_full24(shape, seed):
    """+-2^e * 1.0xxx...x1: 24 significant bits, leading fraction bit 0 (see the module docstring)"""
    g = _g(seed)
    frac = torch.randint(0, 1 << 22, shape, generator=g) | 1                     # 22 free bits, last one set
    return (_pow2(shape, g) * (1.0 + frac.double() * 2.0 ** -23)).float()


def gen_two_plane(shape, seed):
    return _pow2(shape, _g(seed)) * (1.0 + 2.0 ** -10)


def _onehot(values, k_axis, seed):
    """keeps one entry of ``values`` along k_axis (a random position per line), zero elsewhere"""
    g = _g(seed + 7)
    v = values.movedim(k_axis, -1)
    pos = torch.randint(0, v.shape[-1], v.shape[:-1] + (1,), generator=g)
    keep = torch.zeros_like(v).scatter_(-1, pos, 1.0)
    return (v * keep).movedim(-1, k_axis).contiguous()


def family(name, shape_a, ka, shape_b, kb, seed):
    """-> (A, B) storage matrices of the named family; ka / kb: the axis of each that the product reduces over"""
    if name == 'rand6':
        return gen_rand6(shape_a, seed), gen_rand6(shape_b, seed + 1)
    if name == 'ints':
        return gen_ints(shape_a, seed), gen_ints(shape_b, seed + 1)
    base, role = name.rsplit('_', 1)
    dense = {'onehot_full': gen_full24, 'onehot_two_plane': gen_two_plane}[base]
    hot = {'onehot_full': lambda s, sd: _pow2(s, _g(sd)), 'onehot_two_plane': gen_two_plane}[base]
    if role == 'a':
        return _onehot(hot(shape_a, seed), ka, seed), dense(shape_b, seed + 1)
    assert role == 'b'
    return dense(shape_a, seed), _onehot(hot(shape_b, seed + 1), kb, seed)


# ---- the two criteria ----------------------------------------------------------------------------------------------------------
def check_exact(got, ref, what):
    """got (fp32) equals the float64 reference as VALUES (-0 == +0); the reference must be representable"""
    r32 = ref.float()
    assert torch.equal(r32.double(), ref), f'{what}: the reference of an exact family is not representable in fp32 (a test bug)'
    bad = ~(got == r32)
    assert not bool(bad.any()), (f'{what}: exact family missed at {int(bad.sum())} of {bad.numel()} elements, first at '
                                 f'{tuple(int(i) for i in bad.nonzero()[0])}: got {float(got[bad][0])!r}, expected {float(r32[bad][0])!r}')


def check_bound(got, ref, bound, what):
    """|got - ref| <= bound elementwise, NaN fails; -> the largest err / bound"""
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    assert not bool(bad.any()), (f'{what}: derived bound exceeded at {int(bad.sum())} of {bad.numel()} elements, worst err '
                                 f'{float(err[bad].max()):.3e} at bound {float(bound[bad][err[bad].argmax()]):.3e}')
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


class HostBuf:
    """Host twin of hip_testutil._Buf for the CPU tests: a [rows, cols] view with row stride ld in a NaN-filled flat buffer"""
    GUARD = 64

    def __init__(self, rows, cols, ld):
        self.rows, self.cols, self.ld = rows, cols, ld
        self.flat = torch.full((2 * self.GUARD + rows * ld,), float('nan'))

    def view(self, cols=None):
        return torch.as_strided(self.flat, (self.rows, cols or self.cols), (self.ld, 1), self.GUARD)

    def check_untouched(self, written_rows=None, what=''):
        may = torch.zeros(self.flat.shape, dtype=torch.bool)
        mv = torch.as_strided(may, (self.rows, self.cols), (self.ld, 1), self.GUARD)
        if written_rows is None:
            mv[:] = True
        else:
            mv[written_rows] = True
        n = int((~torch.isnan(self.flat[~may])).sum())
        assert n == 0, f'{what}: {n} elements outside the addressed rows / columns were written (guard check)'
        return self.view()
