"""Address arithmetic past 2^31 and 2^32 elements in the dense GEMM family: the fp32 evaluation route writes a [users of a batch,
n_items] score matrix through sbr_gemm_f32 / sbr_gemm_nt_splitk_f32 with ldc = n_items (24,000 users x 90,000 items is past 2^31
elements), and every entry forms ``row * ld`` from an int row or an int32 row map. The scheme of tests/test_hip_big_ld.py: one operand
of each call is a view of at most 130 rows at LD_BIG = 2^25 + 64 inside the one untouched 16.1 GiB buffer, everything else is compact;
every operand that has a leading dimension gets LD_BIG in a case of its own. The big operand has 130 rows where the shape rules allow
it (NT: A big, M = 130; B / W big, N = 130; K-major operands of modes 1 and 2, K = 130; C big, M = 130).

Each case asserts (a) tests/gemm_ref.py's float64 reference under its derived bound (bound_f32 / bound_split, check_exact on the ints
family; nothing new), (b) bit equality with the same call at ld = 192 (256, or 320 for the 258-wide rows, where a row is wider), (c) the guard bands: inputs keep
their bits, and under c_idx the rows of C that the map does not name keep theirs across the full width.

Row maps (a_idx, b_idx, c_idx) are NULL in one case and given in another: permutations of the 130 rows, or injective maps of 120 rows
into the 130 of C; each names rows 0, 63, 64, 65, 127, 128, 129 (asserted before the call). N and K: (136, 64) keeps the generic GEMM on
its float4 / ring path, (134, 66) (K % 4 != 0) sends it to the tile kernel's ragged loads.

Operands that reach only some crossings, or none:
  * W [128, 128] of sbr_gemm_wres_f32, sbr_gemm_split_f32 and sbr_gemm_split_bnstats_f32, W [128, K] of sbr_gemm_split_proj_f32, W
    [K = 128, N] of sbr_gemm_split_wide_f32 mode 1, and C [128, 128] of the bf16-split TN kernel (M a multiple of 128): 128 rows, the
    last one starts past element 2^31 and byte 2^32, not past element 2^32.
  * W [N >= 256, K] of sbr_gemm_split_wide_f32 mode 0 and A, B [K >= 4096, .] of the bf16-split TN kernel hold more rows than the
    buffer has: they reach no crossing here; those entries are tested through their other operands.
sbr_gemm_f32 mode 2 adds with float atomics in arrival order: its cases run the ints family (entries in {-3..3}: every partial sum is
an integer below 2^24, so every order of addition gives the same bits; the premise is checked on the CPU first)."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_ref as R
from big_ld_util import N as NB, both, compact, out, perm_rows, some_rows, unchanged, ws
from hip_testutil import DEV, _BigLd, _i32, _L, _p, act_grad_err, call, ref_act_grad_from_out

pytestmark = pytest.mark.gpu

SHAPES = {'vec': (136, 64), 'ragged': (134, 66)}     # (N, K) of the generic kernels: float4 / ring path, ragged tile-kernel path


@pytest.fixture(scope='module', autouse=True)
def big_buffer():
    """the one large allocation of the module (skips the module when the device has no room for it), freed at the end"""
    _BigLd._flat()
    torch.cuda.reset_peak_memory_stats()
    yield
    print(f'peak device memory of the module: {torch.cuda.max_memory_allocated()} bytes')
    _BigLd.release()


def _lib():
    return _L().lib()


def _arr(ct, vals):
    return ctypes.cast((ct * len(vals))(*vals), ctypes.c_void_p)


def _ref(mode, a, ai, b, bi, bias, M, N, K, act=0):
    fa, fb = a.reshape(-1), b.reshape(-1)
    if mode == 0:
        return R.ref_nt(fa, a.shape[1], ai, fb, b.shape[1], bias, M, N, K, act)
    if mode == 1:
        return R.ref_nn(fa, a.shape[1], ai, fb, b.shape[1], M, N, K, bi)
    return R.ref_tn(fa, a.shape[1], ai, fb, b.shape[1], bi, M, N, K, bias)


def _check(got, ref, pre, Sm, K, act, fam, split, what):
    if fam == 'ints' and act in (0, 1):
        R.check_exact(got, ref, what)
    else:
        r = R.check_bound(got, ref, (R.bound_split if split else R.bound_f32)(Sm, K, ref, pre, act), what)
        print(f'{what}: err / bound {r:.4f}')


def _dims(mode, which, shape, n=None, k=None):
    """M, N, K of a case: 130 on the dimension that counts the big operand's rows, the shape variant elsewhere"""
    N, K = SHAPES[shape] if n is None else (n, k)
    M = NB
    if which == 'B':
        if mode == 0:
            N = NB
        else:
            K = NB
    if which == 'A' and mode == 2:
        K = NB
    if mode == 2 and which == 'C':
        K += 192                           # 256 / 258: a second K range at K = 258, the variant's K % 4 kept
    return M, N, K


def _operands(mode, M, N, K, fam, seed):
    """host storage matrices (A, B) of the product: NT A [M, K] B [N, K]; NN A [M, K] B [K, N]; TN A [K, M] B [K, N]"""
    if mode == 0:
        return R.family(fam, (M, K), 1, (N, K), 1, seed)
    if mode == 1:
        return R.family(fam, (M, K), 1, (K, N), 0, seed)
    return R.family(fam, (K, M), 0, (K, N), 0, seed)


def _perm(seed, n):
    """a permutation of n rows; of the 130 rows of a big operand it names every edge row (asserted)"""
    return perm_rows(seed) if n == NB else np.random.default_rng(seed).permutation(n).astype(np.int64)


def _idx_dev(*maps):
    return tuple(None if v is None else _i32(v) for v in maps)


def _layout(which, make):
    return [(make if which == w else compact) for w in ('A', 'B', 'C')]


# ---- sbr_gemm_f32 -----------------------------------------------------------------------------------------------------------------
def _orders_agree(a, b, what):
    """the premise of an atomic case: the fp32 sum over k taken forwards and backwards equals the float64 sum cast to fp32"""
    fwd, bwd = torch.zeros(a.shape[1], b.shape[1]), torch.zeros(a.shape[1], b.shape[1])
    for k in range(a.shape[0]):
        fwd += a[k][:, None] * b[k][None, :]
        bwd += a[a.shape[0] - 1 - k][:, None] * b[b.shape[0] - 1 - k][None, :]
    ref = (a.double().t() @ b.double()).float()
    assert torch.equal(fwd, ref) and torch.equal(bwd, ref), f'{what}: the inputs do not sum to the same bits in every order'


@pytest.mark.parametrize('maps', [False, True], ids=['identity', 'maps'])
@pytest.mark.parametrize('shape', ['vec', 'ragged'])
@pytest.mark.parametrize('mode,which', [(0, 'A'), (0, 'B'), (0, 'C'), (1, 'A'), (1, 'B'), (1, 'C'), (2, 'A'), (2, 'B'), (2, 'C')])
def test_gemm_f32(mode, which, shape, maps):
    """modes 0 / 1 on the random family (bound_f32), with bias and relu in mode 0; mode 2 (accumulate_atomic = 1) on the ints family into
    a zeroed C. maps: a_idx (a permutation of A's rows: M rows in modes 0 / 1, the k rows in mode 2), b_idx (the k rows of B, modes 1 and
    2), c_idx (mode 0: 120 product rows into the 130 rows of C, so that 10 rows of C are named by nothing)."""
    M, N, K = _dims(mode, which, shape)
    Mp = 120 if (maps and mode == 0) else M                   # product rows
    fam = 'ints' if mode == 2 else 'rand6'
    a, b = _operands(mode, M, N, K, fam, 10 * mode + len(shape))
    bias = R.gen_rand6((N,), 5) if mode == 0 else None
    act = 1 if mode == 0 else 0
    ai = bi = ci = None
    if maps:
        ai = some_rows(Mp, 1) if mode == 0 else _perm(1, K if mode == 2 else M)
        bi = _perm(2, K) if mode in (1, 2) else None
        ci = some_rows(Mp, 3) if mode == 0 else None
    if mode == 2:
        _orders_agree(a if ai is None else a[torch.as_tensor(ai)], b if bi is None else b[torch.as_tensor(bi)], 'sbr_gemm_f32 mode 2')
    ai_d, bi_d, ci_d, bias_d = _idx_dev(ai, bi, ci) + (None if bias is None else bias.to(DEV),)
    what = f'sbr_gemm_f32 mode {mode} {which} {shape} maps={maps}'

    def run(make):
        ma, mb, mc = _layout(which, make)
        Ab, Bb, Cb = ma(*a.shape, a), mb(*b.shape, b), mc(M, N, fill=0.0 if mode == 2 else None)
        call('sbr_gemm_f32', mode, Ab.ptr, Ab.ld, _p(ai_d), Bb.ptr, Bb.ld, _p(bi_d), _p(bias_d), Cb.ptr, Cb.ld, _p(ci_d), Mp, N, K, act,
             1 if mode == 2 else 0, _L().stream())
        unchanged(Ab, a, 'A')
        unchanged(Bb, b, 'B')
        return out(Cb, ci, what=what)

    got = both(run, what)
    ref, pre, Sm = _ref(mode, a, ai, b, bi, bias, Mp, N, K, act)
    _check(got if ci is None else got[torch.as_tensor(ci)], ref, pre, Sm, K, act, fam, False, what)


# ---- sbr_gemm_nt_splitk_f32 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('maps', [False, True], ids=['identity', 'maps'])
@pytest.mark.parametrize('which,N,K', [('A', 136, 256), ('A', 134, 258), ('B', 130, 256), ('B', 130, 258), ('C', 136, 256), ('C', 134, 258)])
def test_gemm_nt_splitk(which, N, K, maps):
    """K = 256 is the shortest reduction the entry splits (two ranges; ring kernel), K = 258 the tile kernel behind it (K % 4 != 0)"""
    M = NB
    Mp = 120 if maps else M
    need = _lib().sbr_gemm_nt_splitk_workspace(Mp, N, K)
    assert need > 0
    a, b = _operands(0, M, N, K, 'rand6', K + N)
    bias = R.gen_rand6((N,), 6)
    ai, ci = (some_rows(Mp, 4), some_rows(Mp, 5)) if maps else (None, None)
    ai_d, ci_d, bias_d = _idx_dev(ai, ci) + (bias.to(DEV),)
    what = f'sbr_gemm_nt_splitk_f32 {which} {N}x{K} maps={maps}'

    def run(make):
        ma, mb, mc = _layout(which, make)
        Ab, Bb, Cb = ma(M, K, a), mb(N, K, b), mc(M, N)
        call('sbr_gemm_nt_splitk_f32', Ab.ptr, Ab.ld, _p(ai_d), Bb.ptr, Bb.ld, _p(bias_d), Cb.ptr, Cb.ld, _p(ci_d), Mp, N, K, 2,
             _p(ws(need)), need, _L().stream())
        unchanged(Ab, a, 'A')
        unchanged(Bb, b, 'B')
        return out(Cb, ci, what=what)

    got = both(run, what)
    ref, pre, Sm = _ref(0, a, ai, b, None, bias, Mp, N, K, 2)
    _check(got if ci is None else got[torch.as_tensor(ci)], ref, pre, Sm, K, 2, 'rand6', False, what)


# ---- sbr_gemm_tn_f32, sbr_gemm_tn_f32_slabs + sbr_splitk_reduce_multi -------------------------------------------------------------
TN_CASES = [('A', 130, 136, 130), ('A', 129, 134, 130), ('B', 132, 136, 130), ('B', 130, 134, 130), ('C', 130, 136, 200), ('C', 130, 134, 203),
            ('C', 128, 128, 4096)]


def _tn_world(which, M, N, K, maps):
    fam = 'rand6'
    a, b = _operands(2, M, N, K, fam, M + N + K)
    ai, bi = (_perm(7, K), _perm(8, K)) if maps else (None, None)
    return a, b, ai, bi


@pytest.mark.parametrize('maps', [False, True], ids=['identity', 'maps'])
@pytest.mark.parametrize('which,M,N,K', TN_CASES)
def test_gemm_tn(which, M, N, K, maps):
    """A [K = 130, M] and B [K = 130, N] K-major at LD_BIG (M, N multiples of 4: the ring; M = 129 / N = 134: the tile kernel); C [130, N]
    crosses both. 128 x 128 x 4096 is served by the bf16-split kernel (bound_split): its C [128, 128] crosses element 2^31 and byte 2^32
    only, and its A, B [4096, 128] hold more rows than the buffer has (no crossing)."""
    a, b, ai, bi = _tn_world(which, M, N, K, maps)
    split = bool(_lib().sbr_gemm_tn_split_supported(M, N, K))
    assert split == (K == 4096)
    need = _lib().sbr_gemm_tn_f32_workspace(M, N, K)
    ai_d, bi_d = _idx_dev(ai, bi)
    what = f'sbr_gemm_tn_f32 {which} {M}x{N}x{K} maps={maps}'

    def run(make):
        ma, mb, mc = _layout(which, make)
        Ab, Bb, Cb = ma(K, M, a), mb(K, N, b), mc(M, N)
        call('sbr_gemm_tn_f32', Ab.ptr, Ab.ld, _p(ai_d), Bb.ptr, Bb.ld, _p(bi_d), Cb.ptr, Cb.ld, M, N, K, _p(ws(need)), need, _L().stream())
        unchanged(Ab, a, 'A')
        unchanged(Bb, b, 'B')
        return out(Cb, what=what)

    got = both(run, what)
    ref, pre, Sm = _ref(2, a, ai, b, bi, None, M, N, K)
    _check(got, ref, pre, Sm, K, 0, 'rand6', split, what)


@pytest.mark.parametrize('maps', [False, True], ids=['identity', 'maps'])
@pytest.mark.parametrize('which,M,N,K', TN_CASES)
def test_gemm_tn_slabs_and_reduce_multi(which, M, N, K, maps):
    """sbr_gemm_tn_f32_slabs has no ldc of its own: the product is finished by sbr_splitk_reduce_multi with ldcs = LD_BIG (the 'C' cases;
    in the 'A' / 'B' cases the slab pass reads the big operand and the reducer writes a compact C). Same shapes as test_gemm_tn."""
    a, b, ai, bi = _tn_world(which, M, N, K, maps)
    split = bool(_lib().sbr_gemm_tn_split_supported(M, N, K))
    need = _lib().sbr_gemm_tn_f32_workspace(M, N, K)
    ai_d, bi_d = _idx_dev(ai, bi)
    what = f'sbr_gemm_tn_f32_slabs + sbr_splitk_reduce_multi {which} {M}x{N}x{K} maps={maps}'

    def run(make):
        ma, mb, mc = _layout(which, make)
        Ab, Bb, Cb, wsb, splits = ma(K, M, a), mb(K, N, b), mc(M, N), ws(need), ctypes.c_int(0)
        call('sbr_gemm_tn_f32_slabs', Ab.ptr, Ab.ld, _p(ai_d), Bb.ptr, Bb.ld, _p(bi_d), M, N, K, _p(wsb), need,
             ctypes.cast(ctypes.pointer(splits), ctypes.c_void_p), _L().stream())
        assert 1 <= splits.value and splits.value * M * N * 4 <= need
        call('sbr_splitk_reduce_multi', 1, _arr(ctypes.c_void_p, [_p(wsb)]), _arr(ctypes.c_void_p, [Cb.ptr]), _arr(ctypes.c_long, [Cb.ld]),
             _arr(ctypes.c_int, [M]), _arr(ctypes.c_int, [N]), _arr(ctypes.c_int, [splits.value]), _L().stream())
        unchanged(Ab, a, 'A')
        unchanged(Bb, b, 'B')
        return out(Cb, what=what)

    got = both(run, what)
    ref, pre, Sm = _ref(2, a, ai, b, bi, None, M, N, K)
    _check(got, ref, pre, Sm, K, 0, 'rand6', split, what)


# ---- sbr_gemm_wres_f32, sbr_gemm_split_f32 (N = K = 128), sbr_gemm_split_bnstats_f32 ------------------------------------------------
@pytest.mark.parametrize('entry', ['wres', 'split'])
@pytest.mark.parametrize('mode,which', [(0, 'A'), (0, 'B'), (0, 'C'), (1, 'A'), (1, 'B'), (1, 'C'), (1, 'Y')])
def test_gemm_wres_and_split(entry, mode, which):
    """N = K = 128 is the one shape sbr_gemm_wres_supported / sbr_gemm_split_supported take (both sides of every term are in
    tests/test_hip_gemm.py::test_wres_split_refusals), M = 130. A, C, Y [130, 128] cross both; W [128, 128] ('B') crosses element 2^31
    and byte 2^32 only. Mode 0 with bias and tanh; mode 1 plain, and in the 'Y' case with the Y epilogue (C = (A W) * relu'(Y)) under the
    bound of tests/test_hip_gemm.py::test_wres_split_y_epilogue_and_colsum."""
    name = {'wres': 'sbr_gemm_wres_f32', 'split': 'sbr_gemm_split_f32'}[entry]
    M, N, K = NB, 128, 128
    assert getattr(_lib(), {'wres': 'sbr_gemm_wres_supported', 'split': 'sbr_gemm_split_supported'}[entry])(M, N, K) == 1
    a, w = _operands(mode, M, N, K, 'rand6', 40 + mode)
    bias = R.gen_rand6((N,), 9) if mode == 0 else None
    act = 2 if mode == 0 else (1 if which == 'Y' else 0)
    y = torch.relu(torch.randn(M, N, generator=torch.Generator().manual_seed(3))) if which == 'Y' else None
    bias_d = None if bias is None else bias.to(DEV)
    what = f'{name} mode {mode} {which}'

    def run(make):
        ma, mb, mc = _layout(which, make)
        Ab, Wb, Cb = ma(M, K, a), mb(128, 128, w), mc(M, N)
        Yb = make(M, N, y) if which == 'Y' else None
        call(name, mode, Ab.ptr, Ab.ld, Wb.ptr, Wb.ld, _p(bias_d), Cb.ptr, Cb.ld, M, N, K, act, Yb.ptr if Yb else None, Yb.ld if Yb else 0, None,
             _L().stream())
        unchanged(Ab, a, 'A')
        unchanged(Wb, w, 'W')
        if Yb:
            unchanged(Yb, y, 'Y')
        return out(Cb, what=what)

    got = both(run, what)
    ref, pre, Sm = _ref(mode, a, None, w, None, bias, M, N, K, 0 if which == 'Y' else act)
    if which == 'Y':
        g = ref_act_grad_from_out(y.double(), act)
        pb = (R.bound_split if entry == 'split' else R.bound_f32)(Sm, K)
        R.check_bound(got, ref * g, pb * g.abs() + ref.abs() * act_grad_err(y.double(), act) + R.U32 * (ref * g).abs() + 1e-300, what)
    else:
        _check(got, ref, pre, Sm, K, act, 'rand6', entry == 'split', what)


@pytest.mark.parametrize('which', ['A', 'B', 'C'])
def test_gemm_split_bnstats(which):
    """the same product (mode 0, N = K = 128, M = 130) with the statistics epilogue: C under bound_split, and C, save_mean, save_rstd
    and the running statistics bit for bit between the two layouts (the statistics are computed from the stored C; their accuracy is the
    subject of tests/test_hip_tail.py). colsum_ws and *arrive are left zeroed. W [128, 128] crosses element 2^31 and byte 2^32 only."""
    M, N, K = NB, 128, 128
    a, w = _operands(0, M, N, K, 'rand6', 50)
    bias = R.gen_rand6((N,), 10)
    bias_d = bias.to(DEV)
    what = f'sbr_gemm_split_bnstats_f32 {which}'

    def run(make):
        ma, mb, mc = _layout(which, make)
        Ab, Wb, Cb = ma(M, K, a), mb(128, 128, w), mc(M, N)
        cws, arrive = torch.zeros(17 * 2 * N, device=DEV, dtype=torch.float64), torch.zeros(1, device=DEV, dtype=torch.int64)
        rm, rv, sm, sr = torch.zeros(N, device=DEV), torch.ones(N, device=DEV), compact(1, N), compact(1, N)
        call('sbr_gemm_split_bnstats_f32', Ab.ptr, Ab.ld, Wb.ptr, Wb.ld, _p(bias_d), Cb.ptr, Cb.ld, M, N, K, 0, _p(cws), _p(arrive), _p(rm), _p(rv),
             None, sm.ptr, sr.ptr, 1e-5, 0.1, _L().stream())
        assert not bool(cws.any()) and int(arrive) == 0
        unchanged(Ab, a, 'A')
        unchanged(Wb, w, 'W')
        return out(Cb, what=what), out(sm, what='save_mean')[0], out(sr, what='save_rstd')[0], rm.cpu(), rv.cpu()

    got, mean, rstd, _, _ = both(run, what)
    ref, pre, Sm = _ref(0, a, None, w, None, bias, M, N, K)
    _check(got, ref, pre, Sm, K, 0, 'rand6', True, what)
    assert bool(torch.isfinite(mean).all()) and bool((rstd > 0).all())


# ---- sbr_gemm_split_proj_f32, sbr_gemm_split_wide_f32 -------------------------------------------------------------------------------
@pytest.mark.parametrize('maps', [False, True], ids=['identity', 'maps'])
@pytest.mark.parametrize('which', ['A', 'B', 'C'])
def test_gemm_split_proj(which, maps):
    """N = 128, K = 256: the smallest shape of sbr_gemm_split_proj_supported (M >= 1 && N == 128 && K >= 256 && K % 128 == 0; both sides
    in tests/test_hip_gemm.py::test_split_proj). A [130, 256] under a_idx and C [130, 128] under c_idx cross both; W [128, 256] crosses
    element 2^31 and byte 2^32 only. A row of A is wider than 192: the small layout is ld = 256."""
    M, N, K = NB, 128, 256
    assert _lib().sbr_gemm_split_proj_supported(M, N, K) == 1
    Mp = 120 if maps else M
    a, w = _operands(0, M, N, K, 'rand6', 60)
    bias = R.gen_rand6((N,), 11)
    ai, ci = (some_rows(Mp, 12), some_rows(Mp, 13)) if maps else (None, None)
    ai_d, ci_d, bias_d = _idx_dev(ai, ci) + (bias.to(DEV),)
    what = f'sbr_gemm_split_proj_f32 {which} maps={maps}'

    def run(make):
        ma, mb, mc = _layout(which, make)
        Ab, Wb, Cb = ma(M, K, a), mb(N, K, w), mc(M, N)
        call('sbr_gemm_split_proj_f32', Ab.ptr, Ab.ld, _p(ai_d), Wb.ptr, Wb.ld, _p(bias_d), Cb.ptr, Cb.ld, _p(ci_d), Mp, N, K, 1, _L().stream())
        unchanged(Ab, a, 'A')
        unchanged(Wb, w, 'W')
        return out(Cb, ci, what=what)

    got = both(run, what)
    ref, pre, Sm = _ref(0, a, ai, w, None, bias, Mp, N, K, 1)
    _check(got if ci is None else got[torch.as_tensor(ci)], ref, pre, Sm, K, 1, 'rand6', True, what)


@pytest.mark.parametrize('maps', [False, True], ids=['identity', 'maps'])
@pytest.mark.parametrize('mode,which,K', [(0, 'A', 64), (0, 'C', 64), (1, 'A', 64), (1, 'B', 128), (1, 'C', 96)])
def test_gemm_split_wide(mode, which, K, maps):
    """N = 256, K in {64, 96, 128}: the smallest shapes of sbr_gemm_split_wide_supported (N % 256 == 0, K >= 64, K % 32 == 0; both sides
    in tests/test_hip_gemm.py::test_split_wide). A [130, K] and C [130, 256] cross both; W [K = 128, 256] of mode 1 crosses element 2^31
    and byte 2^32 only; W [256, K] of mode 0 holds more rows than the buffer has and reaches no crossing: mode 0 is tested through A
    and C. A row of C (and of W in mode 1) is wider than 192: the small layout is ld = 256."""
    M, N = NB, 256
    assert _lib().sbr_gemm_split_wide_supported(M, N, K) == 1
    Mp = 120 if maps else M
    a, w = _operands(mode, M, N, K, 'rand6', 70 + mode)
    bias = R.gen_rand6((N,), 14) if mode == 0 else None
    act = 1 if mode == 0 else 0
    ai, ci = (some_rows(Mp, 15), some_rows(Mp, 16)) if maps else (None, None)
    ai_d, ci_d, bias_d = _idx_dev(ai, ci) + (None if bias is None else bias.to(DEV),)
    what = f'sbr_gemm_split_wide_f32 mode {mode} {which} maps={maps}'

    def run(make):
        ma, mb, mc = _layout(which, make)
        Ab, Wb, Cb = ma(M, K, a), mb(*w.shape, w), mc(M, N)
        call('sbr_gemm_split_wide_f32', mode, Ab.ptr, Ab.ld, _p(ai_d), Wb.ptr, Wb.ld, _p(bias_d), Cb.ptr, Cb.ld, _p(ci_d), Mp, N, K, act,
             _L().stream())
        unchanged(Ab, a, 'A')
        unchanged(Wb, w, 'W')
        return out(Cb, ci, what=what)

    got = both(run, what)
    ref, pre, Sm = _ref(mode, a, ai, w, None, bias, Mp, N, K, act)
    _check(got if ci is None else got[torch.as_tensor(ci)], ref, pre, Sm, K, act, 'rand6', True, what)
