"""References, bounds, fp32 order restatements, input builders and case lists for the dense-block kernels (csrc/block128.h, als.hip,
svd.hip, rbmf.hip, the tail of ease.hip): what tests/test_hip_block_edges.py holds the kernels to and what tests/test_block_refs_cpu.py
shows about these checks without a GPU. numpy and torch only; a plain module: no fixtures, no pytest hooks, no other test module.

Every ``check_*`` takes what a kernel (or a restatement) returned and the inputs as numpy arrays, raises AssertionError, and returns
the worst error / bound ratio (0.0 for a bit comparison). u = 2^-24 is the unit roundoff of fp32. No expected value comes from the
code under test: bit comparisons are against integer arithmetic (exact and order-free by the 2^24 conditions that ``assert_exact_*``
state) followed by single correctly rounded numpy float32 operations; everything else is float64 of the same fp32 inputs.

The bounds (first order in u; each is stated where it is computed):
  rotate        (b + 3) u (|Y||W|)[r, j] / s[j]       b fmaf roundings, the rounding of s, the reciprocal, the final product
  col residual  ((n + slabs) / 2 + 3) u res[j]        see ``col_residual_rel_bound``
  Gram          2 n u (|Y|^T |Y|)[i, j]               the bound of tests/test_hip_svd.py::test_gram: n terms, twice the first-order count
  ALS solve     backward error <= 8 x that of a plain fp32 solve of the same systems (``als_solve32``: sequential accumulation, LAPACK's
                float32 Cholesky, two substitutions), the yardstick rule of tests/als_ref.py restated here
  tri solve     |x T - b| <= gamma_r |x| |T|          Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 8.5
  Cholesky      |R R^T - K| <= gamma_(n+1) |R| |R^T|  Thm 10.3; gamma_k = k u / (1 - k u)

The restatements follow the order that include/sibrar_hip.h states. numpy has no fmaf: ``fma32`` rounds the float64 value of a * b + c
to fp32, which differs from a fused multiply-add only where the float64 sum lands within 2^-29 ulp of an fp32 rounding boundary (a
double rounding); they are used under bounds and on exact integer inputs, never for a bit comparison on rounded data."""
import functools

import numpy as np
import torch

U = 2.0 ** -24
F32 = np.float32
FLT_MIN = F32(2.0 ** -126)
TINY_REL = F32(2.0 ** -46)            # ROT_TINY_REL of csrc/svd.hip
RES_SLAB, GRAM_SLAB = 256, 512       # RES_SLAB of csrc/svd.hip, ALS_G_SLAB of csrc/als.hip
BACKWARD_FACTOR = 8                   # kernel backward error <= 8 x the yardstick's: another summation order, an unblocked factorisation


def gamma(k):
    return k * U / (1 - k * U)


def fma32(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F32)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def same_bits(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == F32 and ref.dtype == F32 and got.shape == ref.shape, f'{what}: {got.dtype} {got.shape} against {ref.dtype} {ref.shape}'
    bad = bits(got) != bits(ref)
    assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.size} elements differ in bits, the first at {tuple(np.argwhere(bad)[0])}'
    return 0.0


def within(got, ref, bound, what):
    """|got - ref| <= bound elementwise in float64, NaN anywhere fails -> the worst ratio"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    bad = ~(err <= bound)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.size} elements over the bound, worst error / bound {ratio:.3f}'
    return ratio


def reduced_cross(rows, widths):
    """every width at two row counts and every row count at two widths (asserted) -> a sorted list of (rows, width)"""
    R = len(rows)
    pairs = set()
    for i, w in enumerate(widths):
        pairs |= {(rows[i % R], w), (rows[(i + R // 2 + 1) % R], w)}
    assert all(sum(1 for p in pairs if p[1] == w) >= 2 for w in widths) and all(sum(1 for p in pairs if p[0] == r) >= 2 for r in rows)
    return sorted(pairs)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- A. sbr_rotate_cols_f32 -----------------------------------------------------------------------------------------------------------
ROT_N = (1, 31, 32, 33, 65)
ROT_B = (1, 7, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128)          # the edges of the four column groups tc, tc + 32, tc + 64, tc + 96
ROT_CASES = reduced_cross(ROT_N, ROT_B)
ROT_INT_MAX = 64                                                    # |y|, |w| <= 64: 128 * 64 * 64 = 2^19 < 2^24
LAM_KINDS = ('relative floor', 'FLT_MIN floor', 'lam[0] zero')


def rotate_s32(lam, tiny_floor=True):
    """s[j] = sqrtf(max(lam[j], max(lam[0] * 2^-46, FLT_MIN))) in float32: product, maxima and root are single correctly rounded (or
    exact) operations, and every candidate that could be subnormal loses against FLT_MIN, so the bits do not depend on how subnormals
    are treated. ``tiny_floor`` False is the mutant without the floor."""
    lam = np.asarray(lam, dtype=F32)
    with np.errstate(invalid='ignore', under='ignore'):
        if not tiny_floor:
            return np.sqrt(lam)
        return np.sqrt(np.maximum(lam, np.maximum(lam[0] * TINY_REL, FLT_MIN)))


def rotate_lam(b, kind, seed):
    """eigenvalue vectors that reach every branch of the floor: exact zeros, negative values, values below lam[0] * 2^-46, and a lam[0] so
    small (or zero) that FLT_MIN is the floor"""
    rng = np.random.default_rng(seed)
    if kind == 'relative floor':
        lam = np.sort(rng.uniform(0.5, 50.0, size=b))[::-1].astype(F32)
        special = [0.0, -1.0, float(lam[0]) * 2.0 ** -50, -0.0, float(lam[0]) * 2.0 ** -46]
    elif kind == 'FLT_MIN floor':
        lam = (rng.uniform(1.0, 2.0, size=b) * 2.0 ** -110).astype(F32)
        lam[0] = F32(1.5 * 2.0 ** -100)                              # lam[0] * 2^-46 = 1.5 * 2^-146, a subnormal below FLT_MIN
        special = [0.0, -2.0 ** -100, 2.0 ** -130, 2.0 ** -126, 2.0 ** -127]
    else:
        lam = rng.uniform(0.5, 50.0, size=b).astype(F32)
        lam[0] = 0.0
        special = [0.0, -3.0, 2.0 ** -140, 2.0 ** -126]
    for k, v in enumerate(special):                                  # from the back, so that lam[0] keeps its role
        if b - 1 - k >= 1:
            lam[b - 1 - k] = F32(v)
    return _frozen(lam)[0]


@functools.lru_cache(maxsize=None)
def rotate_exact_inputs(n, b):
    """integer-valued Y [n, b] and W [b, b] with b * max|y| * max|w| < 2^24: every partial sum of the chain is an integer below 2^24, so
    the fmaf chain is exact in any order"""
    rng = np.random.default_rng(1000 * n + b)
    Y = rng.integers(-ROT_INT_MAX, ROT_INT_MAX + 1, size=(n, b)).astype(F32)
    W = rng.integers(-ROT_INT_MAX, ROT_INT_MAX + 1, size=(b, b)).astype(F32)
    return _frozen(Y, W)


def assert_exact_rotate(Y, W):
    b = Y.shape[1]
    assert np.array_equal(Y, np.rint(Y)) and np.array_equal(W, np.rint(W))
    assert b * float(np.abs(Y).max()) * float(np.abs(W).max()) < 2 ** 24


@functools.lru_cache(maxsize=None)
def rotate_float_inputs(n, b):
    """standard-normal Y, W the orthogonal factor of a random matrix rounded to fp32, lam positive and descending"""
    rng = np.random.default_rng(2000 * n + b)
    Y = rng.standard_normal((n, b)).astype(F32)
    W = np.linalg.qr(rng.standard_normal((b, b)))[0].astype(F32)
    lam = np.sort(rng.uniform(0.5, float(b) + 1.0, size=b))[::-1].astype(F32)
    return _frozen(Y, W, np.ascontiguousarray(lam))


def rotate32(Y, W, lam=None, mutant=None):
    """the header's order in float32: out[r][j] from +0 by fmaf(Y[r][k], W[k][j], .) in ascending k, times 1.0f / s[j] once -> (out, s);
    lam None: the plain product and s None"""
    Y, W = np.asarray(Y, dtype=F32), np.asarray(W, dtype=F32)
    n, b = Y.shape
    s = inv = None
    if lam is not None:
        s = rotate_s32(lam, tiny_floor=mutant != 'no_tiny_floor')
        with np.errstate(divide='ignore', invalid='ignore'):
            inv = F32(1.0) / s
    acc = np.zeros((n, b), dtype=F32)
    with np.errstate(invalid='ignore', over='ignore'):
        for k in range(b):
            w = W[k] * inv if (mutant == 'scale_before_chain' and inv is not None) else W[k]
            acc = fma32(Y[:, k:k + 1], w[None, :], acc)
        out = acc * inv[None, :] if (inv is not None and mutant != 'scale_before_chain') else acc
    if mutant == 'swap_0_64' and b > 64:
        out = out.copy()
        out[:, [0, 64]] = out[:, [64, 0]]
    return out.astype(F32), s


def check_rotate_exact(out, s, Y, W, lam):
    """bit for bit: acc is the exact integer product, out = fl(acc * fl(1 / s[j])), s = ``rotate_s32``; lam None: out = acc and s is not
    looked at"""
    assert_exact_rotate(Y, W)
    acc = (Y.astype(np.int64) @ W.astype(np.int64)).astype(F32)
    if lam is None:
        return same_bits(out, acc, 'rotate, lam NULL')
    s_ref = rotate_s32(lam)
    assert bool((s_ref >= F32(2.0 ** -63)).all())                    # the floor: no s is zero, negative or NaN
    same_bits(s, s_ref, 'rotate: s')
    return same_bits(out, acc * (F32(1.0) / s_ref)[None, :], 'rotate: out')


def check_rotate_float(out, s, Y, W, lam):
    """|out - (Y W)[r, j] / s64[j]| <= (b + 3) u (|Y||W|)[r, j] / s64[j] in float64 of the fp32 inputs: b roundings of the chain (fmaf:
    one per term), one for s = sqrtf(.), one for the reciprocal, one for the final product. s itself bit for bit (a correctly rounded
    root of an fp32 maximum)."""
    b = Y.shape[1]
    same_bits(s, rotate_s32(lam), 'rotate: s')
    lam64 = np.asarray(lam, dtype=np.float64)
    s64 = np.sqrt(np.maximum(lam64, max(lam64[0] * 2.0 ** -46, 2.0 ** -126)))
    Y64, W64 = Y.astype(np.float64), W.astype(np.float64)
    return within(out, (Y64 @ W64) / s64[None, :], (b + 3) * U * (np.abs(Y64) @ np.abs(W64)) / s64[None, :], 'rotate: out')


# ---- B. sbr_col_residual_f32 ----------------------------------------------------------------------------------------------------------
RES_N = (1, 255, 256, 257, 513)
RES_F = (1, 63, 64, 65, 127, 128)
RES_CASES = [(n, f) for n in RES_N for f in RES_F]


def slabs(n, slab):
    return (n + slab - 1) // slab


def col_residual_rel_bound(n):
    """relative bound on res[j]. d = fmaf(-s, u, y) carries one rounding, so d^2 is off by 2u relatively; a term that enters a slab's
    fmaf chain is rounded once per later step of that slab, at most min(n, 256) <= n times; the slab sums are added by at most `slabs`
    rounded additions. All terms are non-negative, so the sum of squares is off by at most (n + slabs + 2) u relatively, first order.
    The root halves that, ((n + slabs) / 2 + 1) u, and sqrtf adds one rounding: ((n + slabs) / 2 + 2) u. One more u covers the second-
    order terms: ((n + slabs + 2) u)^2 / 2 < 5e-10 < u at n <= 513."""
    return ((n + slabs(n, RES_SLAB)) / 2 + 3) * U


@functools.lru_cache(maxsize=None)
def col_residual_inputs(n, f, kind):
    """(Y, U, s, expected or None). 'zero': Y = s U exactly (small integers, s a power of two) -> +0.0. 'squares': Y - s U is a 0/1
    matrix whose column j holds c_j^2 ones, rows 255, 256, 0, n - 1, 511, 512 first -> res[j] = c_j exactly, and a dropped or doubled
    boundary row leaves a non-square. 'float': standard normal. 'cancel': Y within 3 ulp of fl(s U)."""
    rng = np.random.default_rng(3000 * n + 7 * f + len(kind))
    if kind in ('zero', 'squares'):
        Um = rng.integers(-8, 9, size=(n, f)).astype(F32)
        s = (2.0 ** rng.integers(-2, 3, size=f)).astype(F32)
        Y = (s[None, :] * Um).astype(F32)                            # exact: a power of two times an integer
        expected = np.zeros(f, dtype=F32)
        if kind == 'squares':
            cmax = max(c for c in (1, 2, 3, 4) if c * c <= n)
            first = [r for r in (RES_SLAB - 1, RES_SLAB, 0, n - 1, 2 * RES_SLAB - 1, 2 * RES_SLAB) if 0 <= r < n]
            first = list(dict.fromkeys(first))
            for j in range(f):
                c = 1 if cmax == 1 else 2 + j % (cmax - 1)           # at least four ones where there is room (both boundary rows);
                                                                     # columns 0 and 64 differ (64 % 3 = 1)
                rest = [r for r in rng.permutation(n) if r not in first]
                rows = (first + rest)[:c * c]
                Y[rows, j] += F32(1.0)
                expected[j] = c
        return _frozen(Y, Um, s, expected)
    Um = rng.standard_normal((n, f)).astype(F32)
    s = rng.uniform(0.5, 4.0, size=f).astype(F32)
    if kind == 'float':
        Y = rng.standard_normal((n, f)).astype(F32)
    else:
        Y = (s[None, :] * Um).astype(F32)
        for _ in range(3):
            step = rng.integers(-1, 2, size=(n, f))
            Y = np.where(step > 0, np.nextafter(Y, F32(np.inf)), np.where(step < 0, np.nextafter(Y, F32(-np.inf)), Y)).astype(F32)
    return _frozen(Y, Um, s) + (None,)


def assert_exact_col_residual(Y, Um, s):
    d = Y.astype(np.float64) - s.astype(np.float64)[None, :] * Um.astype(np.float64)
    assert np.array_equal(d, np.rint(d)) and float((d * d).sum(axis=0).max()) < 2 ** 24
    assert np.array_equal(np.log2(s), np.rint(np.log2(s)))


def col_residual32(Y, Um, s, mutant=None):
    """the header's order in float32: d = fmaf(-s[j], U[r][j], Y[r][j]), acc = fmaf(d, d, acc) in ascending r within slabs of 256 from
    +0, the slabs' sums added in slab order from +0, one sqrtf"""
    n, f = Y.shape
    total = np.zeros(f, dtype=F32)
    for lo in range(0, n, RES_SLAB):
        hi = min(lo + RES_SLAB, n)
        rows = list(range(lo, hi))
        if mutant == 'drop_last_of_slab' and hi - lo == RES_SLAB:
            rows = rows[:-1]
        if mutant == 'double_first_of_slab' and lo > 0:
            rows = [lo] + rows
        acc = np.zeros(f, dtype=F32)
        for r in rows:
            d = fma32(-s, Um[r], Y[r])
            acc = fma32(d, d, acc)
        total = (total + acc).astype(F32)
    res = np.sqrt(total)
    if mutant == 'swap_0_64' and f > 64:
        res[[0, 64]] = res[[64, 0]]
    return res


def check_col_residual_exact(res, Y, Um, s, expected):
    assert_exact_col_residual(Y, Um, s)
    d = Y.astype(np.float64) - s.astype(np.float64)[None, :] * Um.astype(np.float64)
    assert np.array_equal((d * d).sum(axis=0), expected.astype(np.float64) ** 2)          # the builder's claim, from the data
    return same_bits(res, expected, 'col residual (exact)')


def check_col_residual_float(res, Y, Um, s):
    n = Y.shape[0]
    ref = np.sqrt(((Y.astype(np.float64) - s.astype(np.float64)[None, :] * Um.astype(np.float64)) ** 2).sum(axis=0))
    return within(res, ref, col_residual_rel_bound(n) * ref, 'col residual')


# ---- C. sbr_ease_weights_f32 ----------------------------------------------------------------------------------------------------------
EASE_N = (1, 2, 255, 256, 257, 300)
EASE_N_WRAP = 4097                    # the row loop i += gridDim.y wraps from n = 4097 on


@functools.lru_cache(maxsize=2)
def ease_inputs(n):
    """a deliberately non-symmetric P with a non-zero diagonal of mixed sign"""
    rng = np.random.default_rng(4000 + n)
    P = rng.standard_normal((n, n), dtype=F32)
    d = rng.uniform(0.5, 2.0, size=n).astype(F32)
    d[::2] *= F32(-1.0)
    P[np.arange(n), np.arange(n)] = d
    return _frozen(P)[0]


def ease_weights32(P, mutant=None):
    """B[i][j] = float32(P[i][j]) / float32(-P[j][j]), one correctly rounded division; +0.0 on the diagonal"""
    d = -np.diagonal(P).astype(F32)
    out = (P / (d[:, None] if mutant == 'row_diagonal' else d[None, :])).astype(F32)
    out[np.arange(len(d)), np.arange(len(d))] = F32(0.0)
    return out


def check_ease(got, P):
    n = P.shape[0]
    ref = ease_weights32(P)
    same_bits(got, ref, 'ease weights')
    if n > 1:                                                        # explicitly: the column's diagonal, not the row's
        by_row = ease_weights32(P, 'row_diagonal')
        off = ~np.eye(n, dtype=bool)
        differ = bits(by_row)[off] != bits(ref)[off]
        assert differ.mean() > 0.9, 'the input does not tell the column rule from the row rule'
        assert bool((bits(got)[off][differ] != bits(by_row)[off][differ]).all()), 'divided by the row\'s diagonal element'
    return 0.0


# ---- D. the Gram entries --------------------------------------------------------------------------------------------------------------
GRAM_N = (511, 512, 513, 1024, 1025)
GRAM_F = (1, 8, 9, 63, 64, 65, 127, 128)
GRAM_CASES = reduced_cross(GRAM_N, GRAM_F)
GRAM_FLOAT_CASES = [(511, 9), (512, 128), (513, 63), (1024, 65), (1025, 127)]          # one float case per row count
GRAM_REG = 0.1                        # not a dyadic number: the last addition rounds


@functools.lru_cache(maxsize=None)
def gram_inputs(n, f, kind):
    """'int': integers in [-4, 4], row k non-zero in column k % f (its signature: no row is zero, so dropping or doubling any row
    changes a diagonal element). 'float': standard normal."""
    rng = np.random.default_rng(5000 * n + f)
    if kind == 'float':
        return _frozen(rng.standard_normal((n, f)).astype(F32))[0]
    Y = rng.integers(-4, 5, size=(n, f)).astype(F32)
    k = np.arange(n)
    Y[k, k % f] = (1 + k % 4) * np.where(k % 3 == 0, -1, 1)
    return _frozen(Y)[0]


def assert_exact_gram(Y):
    assert np.array_equal(Y, np.rint(Y)) and float(np.abs(Y).max()) <= 4 and Y.shape[0] * 16 < 2 ** 24
    assert bool((np.abs(Y).sum(axis=1) > 0).all())


def gram32(Y, reg=0.0, mutant=None):
    """the header's order in float32: G[i][j] from +0 by fmaf(Y[k][i], Y[k][j], .) in ascending k within slabs of 512, the slabs' sums
    added in slab order from +0, reg added to the diagonal last"""
    n, f = Y.shape
    if mutant == 'swap_0_64' and f > 64:
        Y = Y.copy()
        Y[:, [0, 64]] = Y[:, [64, 0]]
    total = np.zeros((f, f), dtype=F32)
    for lo in range(0, n, GRAM_SLAB):
        hi = min(lo + GRAM_SLAB, n)
        rows = list(range(lo, hi))
        if mutant == 'drop_last_of_slab' and hi - lo == GRAM_SLAB:
            rows = rows[:-1]
        if mutant == 'double_first_of_slab' and lo > 0:
            rows = [lo] + rows
        acc = np.zeros((f, f), dtype=F32)
        for r in rows:
            acc = fma32(Y[r][:, None], Y[r][None, :], acc)
        total = (total + acc).astype(F32)
    if reg:
        total[np.arange(f), np.arange(f)] += F32(reg)
    return total


def _gram_symmetric(G):
    assert np.array_equal(bits(G), bits(G.T)), 'G is not symmetric bit for bit'


def check_gram_exact(G, Y, reg=0.0):
    """bit for bit: float32(Y^T Y) from integer arithmetic, plus float32(reg) on the diagonal as one rounded addition"""
    assert_exact_gram(Y)
    ref = (Y.astype(np.int64).T @ Y.astype(np.int64)).astype(F32)
    if reg:
        ref[np.arange(len(ref)), np.arange(len(ref))] += F32(reg)
    _gram_symmetric(G)
    return same_bits(G, ref, f'gram {Y.shape} reg={reg}')


def check_gram_float(G, Y, reg=0.0):
    """the bound of tests/test_hip_svd.py::test_gram, 2 n u |Y|^T |Y|; with reg, one more rounding of the diagonal element"""
    n = Y.shape[0]
    Y64 = Y.astype(np.float64)
    ref = Y64.T @ Y64 + float(F32(reg)) * np.eye(Y.shape[1])
    _gram_symmetric(G)
    last = U * np.abs(ref) * np.eye(Y.shape[1]) if reg else 0.0
    return within(G, ref, 2 * n * U * (np.abs(Y64).T @ np.abs(Y64)) + last, f'gram {Y.shape}')


# ---- E. the row solvers ---------------------------------------------------------------------------------------------------------------
ALS_F = (1, 63, 64, 65, 127, 128)
ALS_NY = 70                           # not a multiple of the staging chunk: the full row is staged as 24 + 24 + 22
ALS_ROW_NNZ = (3, 0, 1, 23, 24, 25, 47, 48, 49, ALS_NY, 5)          # the staging edges of a 24-row chunk; row 1 is the empty one
ALS_ALPHA, ALS_REG = 40.0, 0.01
TRI_R, TRI_N = (63, 64, 65, 127), 5
CHOL_N = (63, 64, 127)


@functools.lru_cache(maxsize=None)
def als_world(weighted):
    """CSR (indptr int64, indices int32 ascending and unique, data float32 or None) whose rows hold exactly ALS_ROW_NNZ entries"""
    rng = np.random.default_rng(61 + weighted)
    indptr = np.concatenate([[0], np.cumsum(ALS_ROW_NNZ)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(ALS_NY, size=k, replace=False)) for k in ALS_ROW_NNZ]).astype(np.int32)
    data = rng.integers(1, 6, size=len(indices)).astype(F32) if weighted else None
    assert list(np.diff(indptr)) == list(ALS_ROW_NNZ)
    return _frozen(indptr, indices) + (None if data is None else _frozen(data)[0],)


@functools.lru_cache(maxsize=None)
def als_factors(f):
    """(Y uniform(-0.5 / f, 0.5 / f) as tests/als_ref.py draws it, G = float32(Y^T Y + reg I) from float64: an input of the solver)"""
    Y = np.random.default_rng(70 + f).uniform(-0.5 / f, 0.5 / f, size=(ALS_NY, f)).astype(F32)
    Y64 = Y.astype(np.float64)
    return _frozen(Y, (Y64.T @ Y64 + ALS_REG * np.eye(f)).astype(F32))


def als_system64(world, r, Y, G, alpha):
    """(A_r, b_r) in float64 from the fp32 inputs; c = alpha * r as the fp32 product the header states"""
    indptr, indices, data = world
    cols = indices[indptr[r]:indptr[r + 1]]
    vals = np.ones(len(cols), dtype=F32) if data is None else data[indptr[r]:indptr[r + 1]]
    c = (F32(alpha) * vals).astype(np.float64)
    ys = Y[cols].astype(np.float64)
    return G.astype(np.float64) + (ys * (c - 1.0)[:, None]).T @ ys, (ys * c[:, None]).sum(axis=0)


def tri_solve32(b, T, upper, unit, mutant=None):
    """x T = b row by row in float32 in the header's order: lower T, j descending (upper: ascending): x_j = b_j / T_jj, then
    b_m = fmaf(-x_j, T[j][m], b_m) for m < j (upper: m > j)"""
    x = np.array(b, dtype=F32)
    r = x.shape[1]
    for j in (range(r) if upper else range(r - 1, -1, -1)):
        if not unit:
            x[:, j] = x[:, j] / T[j, j]
        m = slice(j + 1, r) if upper else slice(0, j)
        x[:, m] = fma32(-x[:, j:j + 1], T[j, m][None, :], x[:, m])
    if mutant == 'swap_0_64' and r > 64:
        x[:, [0, 64]] = x[:, [64, 0]]
    return x


def chol32(K):
    """Cholesky by columns in float32 in the header's order: q and s_i as fmaf chains in ascending k, R[p][p] = sqrtf(q),
    R[i][p] = s_i / R[p][p]; zeros above the diagonal"""
    n = K.shape[0]
    A = np.tril(K).astype(F32)
    R = np.zeros((n, n), dtype=F32)
    for p in range(n):
        s = A[p:, p].copy()
        for k in range(p):
            s = fma32(-R[p:, k], R[p, k], s)
        R[p, p] = np.sqrt(s[0])
        R[p + 1:, p] = s[1:] / R[p, p]
    return R


def als_solve32(world, Y, G, alpha):
    """the yardstick: float32 throughout, the row's terms added one after the other in CSR order (plain products and sums), LAPACK's
    float32 Cholesky (numpy.linalg.cholesky on float32), then the two substitutions in float32. An empty row is zeros."""
    indptr, indices, data = world
    n, f = len(indptr) - 1, Y.shape[1]
    out = np.zeros((n, f), dtype=F32)
    for r in range(n):
        if indptr[r + 1] == indptr[r]:
            continue
        A, b = G.astype(F32).copy(), np.zeros(f, dtype=F32)
        for p in range(indptr[r], indptr[r + 1]):
            y, c = Y[indices[p]], F32(alpha) * (F32(1.0) if data is None else data[p])
            A += np.outer((c - F32(1.0)) * y, y)
            b += c * y
        L = np.linalg.cholesky(A)
        assert L.dtype == F32
        z = tri_solve32(b[None, :], np.ascontiguousarray(L.T), upper=True, unit=False)       # z L^T = b, that is L z = b
        out[r] = tri_solve32(z, L, upper=False, unit=False)[0]                                # x L = z, that is L^T x = z
    return out


def als_backward_error(world, Y, G, alpha, got):
    """max over the non-empty rows of ||A_r x_r - b_r||_inf / (||A_r||_inf ||x_r||_inf + ||b_r||_inf) in float64 from the fp32 inputs"""
    indptr = world[0]
    got = np.asarray(got, dtype=np.float64)
    worst = 0.0
    for r in range(len(indptr) - 1):
        if indptr[r + 1] == indptr[r]:
            continue
        a, b = als_system64(world, r, Y, G, alpha)
        res = np.abs(a @ got[r] - b).max()
        assert np.isfinite(res), f'row {r} is not finite'
        worst = max(worst, res / (np.abs(a).sum(axis=1).max() * np.abs(got[r]).max() + np.abs(b).max()))
    return worst


@functools.lru_cache(maxsize=None)
def als_yardstick(f, weighted):
    Y, G = als_factors(f)
    return als_backward_error(als_world(weighted), Y, G, ALS_ALPHA, als_solve32(als_world(weighted), Y, G, ALS_ALPHA))


def check_als(X, f, weighted):
    """the checks of tests/test_hip_als.py::test_half_sweep on the staging-edge world: backward error <= BACKWARD_FACTOR x the
    yardstick's, finite, the empty row +0.0 in every bit -> kernel / (BACKWARD_FACTOR x yardstick)"""
    Y, G = als_factors(f)
    world = als_world(weighted)
    empty = np.flatnonzero(np.diff(world[0]) == 0)
    assert len(empty) == 1 and np.isfinite(X).all()
    assert not bits(X[empty]).any(), 'the empty row is not +0.0f bit for bit'
    be, be_ref = als_backward_error(world, Y, G, ALS_ALPHA, X), als_yardstick(f, weighted)
    assert be <= BACKWARD_FACTOR * be_ref, f'backward error {be:.3e}, yardstick {be_ref:.3e}'
    return be / (BACKWARD_FACTOR * be_ref)


def als_restated32(f, weighted, mutant=None):
    """the header's order in float32 for the CPU module: A_r from G by fmaf((c - 1) y[i], y[j], .), b_r by fmaf(c, y[i], .) in CSR
    order, Cholesky by columns (``chol32``), the substitutions of ``tri_solve32``"""
    Y, G = als_factors(f)
    indptr, indices, data = als_world(weighted)
    out = np.zeros((len(indptr) - 1, f), dtype=F32)
    for r in range(len(indptr) - 1):
        if indptr[r + 1] == indptr[r]:
            continue
        A, b = G.copy(), np.zeros(f, dtype=F32)
        for p in range(indptr[r], indptr[r + 1]):
            y, c = Y[indices[p]], F32(ALS_ALPHA) * (F32(1.0) if data is None else data[p])
            A = fma32(((c - F32(1.0)) * y)[:, None], y[None, :], A)
            b = fma32(c, y, b)
        L = chol32(A)
        z = tri_solve32(b[None, :], np.ascontiguousarray(L.T), upper=True, unit=False)
        out[r] = tri_solve32(z, L, upper=False, unit=False)[0]
    if mutant == 'swap_0_64' and f > 64:
        out[:, [0, 64]] = out[:, [64, 0]]
    return out


@functools.lru_cache(maxsize=None)
def tri_inputs(r):
    """(b [TRI_N, r] standard normal, a full matrix T whose triangles are well conditioned: off-diagonal N(0, 1 / r), |diagonal| in
    [1, 2] of mixed sign); five rows: a wave owns a row, so the second workgroup of four waves is partly filled"""
    rng = np.random.default_rng(80 + r)
    b = rng.standard_normal((TRI_N, r)).astype(F32)
    T = (rng.standard_normal((r, r)) / np.sqrt(r)).astype(F32)
    T[np.arange(r), np.arange(r)] = rng.uniform(1, 2, size=r).astype(F32) * rng.choice([-1, 1], size=r).astype(F32)
    return _frozen(b, T)


def check_tri(x, b, T, upper, unit):
    r = T.shape[0]
    t64 = (np.triu(T) if upper else np.tril(T)).astype(np.float64)
    if unit:
        t64[np.arange(r), np.arange(r)] = 1.0
    x64 = np.asarray(x, dtype=np.float64)
    return within(x64 @ t64, b.astype(np.float64), gamma(r) * (np.abs(x64) @ np.abs(t64)), f'tri solve r={r} upper={upper} unit={unit}')


@functools.lru_cache(maxsize=None)
def chol_input(n):
    """C C^T + 0.01 I for a 0/1 matrix C, the ridge system of tests/test_hip_rbmf.py::test_cholesky"""
    c = (np.random.default_rng(90 + n).random((n, 3 * n + 5)) < 0.3).astype(F32)
    return _frozen((c @ c.T + F32(1e-2) * np.eye(n, dtype=F32)).astype(F32))[0]


def check_chol(R, K):
    n = K.shape[0]
    assert not bits(np.triu(R, 1)).any(), 'R is not +0.0 above the diagonal'
    assert bool((np.diagonal(R) > 0).all())
    R64 = np.asarray(R, dtype=np.float64)
    return within(R64 @ R64.T, K.astype(np.float64), gamma(n + 1) * (np.abs(R64) @ np.abs(R64.T)), f'cholesky n={n}')


def as_torch(a):
    return torch.from_numpy(np.array(a, order='C'))                 # a copy: the builders' arrays are read-only
