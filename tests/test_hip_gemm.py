"""The dense GEMM family against float64 (tests/gemm_ref.py: references, derived bounds, exact operand families), called through the
C ABI with operands inside NaN-filled buffers (hip_testutil._Buf): leading dimensions larger than the row, guards in front, behind and
between rows, check_untouched on C and on the workspace after every call. Every case's comment quotes the dispatch condition of the
.hip source it sits on or breaks. Every case runs the `ints` family (exact) and the random six-decade family (bound); cases with
M N K <= ONEHOT_BUDGET (3e8) also run the one-hot families — onehot_full on every entry: sbr_gemm_f32 in all three modes (every case but
the 80k-row and long-gathered-range ones), sbr_gemm_nt_splitk_f32 (all but 4096 x 128 x 2048), sbr_gemm_tn_f32 on the ring, tile and split
kernels (all but the k_chunk-cap and K = 600,000 cases), wres / split (M <= 65), proj (all but the 65k-row case), wide (M <= 300);
onehot_two_plane on the bf16-split entries split, proj, wide and the split TN kernel, in those same cases; every
fixed-order entry is called twice on the random family and compared in bits. Epilogues with a transcendental (tanh, sigmoid, selu)
have no exactly representable result: there the exact families are held to the activation bound instead.
RATIOS collects the largest err / bound per entry point on the random family (printed by the last test; DESIGN.md quotes a run)."""
import ctypes
import json

import numpy as np
import pytest
import torch

import gemm_ref as R
from hip_testutil import DEV, GUARD, S, _L, _assert_bits, _Buf, _i32, _p, act_grad_err, call, ref_act_grad_from_out, stream

pytestmark = pytest.mark.gpu
RATIOS = {}
SPLIT_ENTRIES = ('split', 'proj', 'wide')
ONEHOT_BUDGET = 3e8                          # M N K up to which a case also runs the one-hot families


def _lib():
    return _L().lib()


def _err():
    return _L().SibrarHipError


def _flat(buf):
    """host copy of the buffer from the view's base on (what the C entry's pointer sees)"""
    return buf.flat.cpu()[GUARD + buf.off:]


def _ws(nbytes):
    assert nbytes % 4 == 0
    return _Buf(1, max(nbytes // 4, 1))


def _idx_repeats(n, n_table, seed):
    r = np.random.default_rng(seed).integers(0, n_table, size=n)
    r[: min(n, 3)] = np.arange(min(n, 3)) % n_table
    return r


def _idx_injective(n, n_table, seed):
    return np.random.default_rng(seed).permutation(n_table)[:n]


def _fams(entry, M, N, K):
    fams = ['ints', 'rand6']
    if M * N * K <= ONEHOT_BUDGET:
        fams += ['onehot_full_a', 'onehot_full_b']
        if entry in SPLIT_ENTRIES or entry == 'tn_split':
            fams += ['onehot_two_plane_a', 'onehot_two_plane_b']
    return fams


def _tn_splits(M, N, K):
    """tn_splits of csrc/gemm_f32.hip (the slab count of the fp32 kernels), for workspaces sized to it alone"""
    cd = lambda a, b: -(-a // b)
    tiles = cd(M, 64) * cd(N, 128)
    want = cd(1536 if tiles >= 8 else 512, tiles)
    splits = max(min(want, cd(K, 128)), cd(K, 512))
    return max(splits, 1)


def _slabs_f32(M, N, K):
    """slabs the fp32 ring / tile kernels write (tn_slabs: k_chunk rounded up to whole slabs of 32, then the count re-cut)"""
    cd = lambda a, b: -(-a // b)
    return cd(K, cd(cd(K, _tn_splits(M, N, K)), 32) * 32)


def _slabs_split(M, N, K):
    """sbr_tn_split_splits of csrc/gemm_split_tn_f32.hip for an eligible shape (TS_KC = 32, 64 chunks per range at most)"""
    cd = lambda a, b: -(-a // b)
    chunks = cd(K, 32)
    return min(max(256 // ((N // 128) * (M // 128)), cd(chunks, 64), 1), chunks) if M % 128 == 0 and N % 128 == 0 and M and N else 0


def run(entry, mode, M, N, K, *, gather=False, scatter=False, bias=False, act=0, pa=4, pb=4, pc=3, oa=0, ob=0, oc=0, fams=None,
        ws_bytes=None, seed=0, expect_split=None):
    """One product through ``entry`` for every operand family of the case; -> nothing (asserts).
    entry: 'f32' (sbr_gemm_f32, mode 0 / 1 / 2), 'nt_splitk', 'tn', 'tn_split' (sbr_gemm_tn_f32 served by the bf16-split kernel), 'wres',
    'split', 'proj', 'wide'. gather: True (a_idx; in TN also b_idx), 'a' (a_idx alone), 'b' (b_idx alone: TN, and mode 1 of 'f32', whose b_idx maps B's k rows)
    or 'ab' (both, for that mode 1);
    scatter: c_idx into a larger C. bias in mode 2 exists for 'f32' only."""
    tn = mode == 2
    pipe_split = entry in SPLIT_ENTRIES or entry == 'tn_split'
    name = {'f32': 'sbr_gemm_f32', 'nt_splitk': 'sbr_gemm_nt_splitk_f32', 'tn': 'sbr_gemm_tn_f32', 'tn_split': 'sbr_gemm_tn_f32',
            'wres': 'sbr_gemm_wres_f32', 'split': 'sbr_gemm_split_f32', 'proj': 'sbr_gemm_split_proj_f32', 'wide': 'sbr_gemm_split_wide_f32'}[entry]
    if expect_split is not None:
        assert _lib().sbr_gemm_tn_split_supported(M, N, K) == expect_split
    for fi, fam in enumerate(fams or _fams(entry, M, N, K)):
        what = f'{name} mode {mode} {M}x{N}x{K} [{fam}]'
        exact = fam != 'rand6'
        onehot = fam.startswith('onehot')
        sd = seed + 17 * fi
        # ---- storage: A [rows_a, wa], B [rows_b, wb]; a one-hot operand is built in product order and scattered to its table through
        # an injective map (repeated rows would put several non-zeros into one reduction); the other families repeat rows heavily
        ga = gather in (True, 'a', 'ab')
        gb = gather in (True, 'b', 'ab') if tn else (gather in ('b', 'ab') and mode == 1 and entry == 'f32')

        def table(logical, rows, gathered, frac, sd_):
            if not gathered:
                return logical, None
            if onehot:
                idx = _idx_injective(rows, rows + 5, sd_)
                t = torch.zeros(rows + 5, logical.shape[1])
                t[torch.as_tensor(idx)] = logical
                return t, idx
            idx = _idx_repeats(rows, rows // frac + 1, sd_)
            return None, idx                                        # the table is drawn directly (below)

        if tn:
            la, lb = R.family(fam, (K, M), 0, (K, N), 0, sd)
            a, ai = table(la, K, ga, 3, sd)
            b, bi = table(lb, K, gb, 2, sd + 1)
            if a is None or b is None:
                ta, tb = R.family(fam, (K // 3 + 1 if a is None else 1, M), 0, (K // 2 + 1 if b is None else 1, N), 0, sd + 5)
                a, b = (ta if a is None else a), (tb if b is None else b)
        else:
            n_ta = M // 3 + 1 if ga else M
            ai = _idx_repeats(M, n_ta, sd) if ga else None
            a, lb = R.family(fam, (n_ta, K), 1, (N, K) if mode == 0 else (K, N), 1 if mode == 0 else 0, sd)
            b, bi = table(lb, K, gb, 2, sd + 1)
            if b is None:
                b = R.family(fam, (1, K), 1, (K // 2 + 1, N), 0, sd + 5)[1]
        bias_t = None
        if bias:
            bias_t = R.gen_rand6((N,), sd + 2) if fam == 'rand6' else (R.gen_int_bias(N, sd + 2) if fam == 'ints' else torch.zeros(N))
        Ab = _Buf(a.shape[0], a.shape[1], ld=a.shape[1] + pa, off=oa, data=a)
        Bb = _Buf(b.shape[0], b.shape[1], ld=b.shape[1] + pb, off=ob, data=b)
        c_rows = M + M // 4 + 2 if scatter else M
        ci = _idx_injective(M, c_rows, sd + 3) if scatter else None
        ai_d, bi_d, ci_d = (None if x is None else _i32(x) for x in (ai, bi, ci))
        bias_d = None if bias_t is None else bias_t.to(DEV)

        def once():
            Cb = _Buf(c_rows, N, ld=N + pc, off=oc)
            wsb = None
            if entry == 'f32':
                if tn:
                    Cb.t.zero_()                                    # mode 2 accumulates into a zeroed C (the guards stay NaN)
                call(name, mode, Ab.ptr, Ab.ld, _p(ai_d), Bb.ptr, Bb.ld, _p(bi_d), _p(bias_d), Cb.ptr, Cb.ld, _p(ci_d), M, N, K, act,
                     1 if tn else 0, stream())
            elif entry == 'nt_splitk':
                need = _lib().sbr_gemm_nt_splitk_workspace(M, N, K)
                assert need > 0, f'{what}: the case must be a split shape'
                wsb = _ws(need)
                call(name, Ab.ptr, Ab.ld, _p(ai_d), Bb.ptr, Bb.ld, _p(bias_d), Cb.ptr, Cb.ld, _p(ci_d), M, N, K, act, wsb.ptr, need, stream())
            elif entry in ('tn', 'tn_split'):
                need = _lib().sbr_gemm_tn_f32_workspace(M, N, K) if ws_bytes is None else ws_bytes
                wsb = _ws(need)
                call(name, Ab.ptr, Ab.ld, _p(ai_d), Bb.ptr, Bb.ld, _p(bi_d), Cb.ptr, Cb.ld, M, N, K, wsb.ptr, need, stream())
            elif entry in ('wres', 'split'):
                call(name, mode, Ab.ptr, Ab.ld, Bb.ptr, Bb.ld, _p(bias_d), Cb.ptr, Cb.ld, M, N, K, act, None, 0, None, stream())
            elif entry == 'proj':
                call(name, Ab.ptr, Ab.ld, _p(ai_d), Bb.ptr, Bb.ld, _p(bias_d), Cb.ptr, Cb.ld, _p(ci_d), M, N, K, act, stream())
            else:
                call(name, mode, Ab.ptr, Ab.ld, _p(ai_d), Bb.ptr, Bb.ld, _p(bias_d), Cb.ptr, Cb.ld, _p(ci_d), M, N, K, act, stream())
            if wsb is not None:
                wsb.check_untouched(what=what + ' workspace')      # nothing in front of the workspace or behind workspace_bytes
            host = Cb.check_untouched(written_rows=ci, what=what)
            return host if ci is None else host[torch.as_tensor(ci)]

        got = once()
        if entry in ('tn', 'tn_split'):
            # which kernel served the call: sbr_gemm_tn_f32_slabs runs the same dispatch and reports the slab count, which differs
            # between the fp32 kernels (tn_splits, re-cut to whole slabs of 32) and the bf16-split kernel (sbr_tn_split_splits)
            need = _lib().sbr_gemm_tn_f32_workspace(M, N, K) if ws_bytes is None else ws_bytes
            wsb, so = _ws(need), ctypes.c_int(0)
            call('sbr_gemm_tn_f32_slabs', Ab.ptr, Ab.ld, _p(ai_d), Bb.ptr, Bb.ld, _p(bi_d), M, N, K, wsb.ptr, need,
                 ctypes.cast(ctypes.pointer(so), ctypes.c_void_p), stream())
            want_f32, want_split = _slabs_f32(M, N, K), _slabs_split(M, N, K)
            assert want_f32 != want_split, f'{what}: the slab counts of the two kernels must differ for the case to pin the dispatch'
            assert so.value == (want_split if entry == 'tn_split' else want_f32), \
                f'{what}: {so.value} slabs, the {"bf16-split" if entry == "tn_split" else "fp32"} kernel writes {want_split if entry == "tn_split" else want_f32}'
        fa, fb = _flat(Ab), _flat(Bb)
        if mode == 0:
            ref, pre, Sm = R.ref_nt(fa, Ab.ld, ai, fb, Bb.ld, bias_t, M, N, K, act)
        elif mode == 1:
            ref, pre, Sm = R.ref_nn(fa, Ab.ld, ai, fb, Bb.ld, M, N, K, bi)
        else:
            ref, pre, Sm = R.ref_tn(fa, Ab.ld, ai, fb, Bb.ld, bi, M, N, K, bias_t)
        bound = (R.bound_split if pipe_split else R.bound_f32)(Sm, K, ref, pre, act)
        if exact and act in (0, 1):
            R.check_exact(got, ref, what)
        else:
            ratio = R.check_bound(got, ref, bound, what)
            if fam == 'rand6':
                RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
                print(f'{what}: err / bound {ratio:.4f}')
        if fam == 'rand6' and not (entry == 'f32' and tn):          # documented as fixed-order: the same bits on a second call
            _assert_bits(once(), got, what + ' second call')


# =================================================================================================================================
# sbr_gemm_f32, modes 0 and 1
# =================================================================================================================================
@pytest.mark.parametrize('mode', (0, 1))
def test_gemm_f32_ring_eligibility(mode):
    # ring eligible: ring_al16(g.A, g.lda) && ring_al16(g.B, g.ldb), K % 4 == 0, K >= BK; ragged M and N on the 64 x 128 ring tile
    run('f32', mode, 200, 136, 64, bias=mode == 0, gather=True)
    # !ring_al16(g.A, g.lda): A 4 bytes off the 16-byte boundary (also vecA = 0 in the tile kernel: the scalar loads of load_mk)
    run('f32', mode, 200, 136, 64, oa=1, gather=True)
    # !ring_al16(g.A, g.lda): A 8 bytes off
    run('f32', mode, 200, 136, 64, oa=2)
    # !ring_al16(g.B, g.ldb): B off alignment (vecB = 0: scalar loads of load_mk / load_km)
    run('f32', mode, 200, 136, 64, ob=1)
    # !ring_al16(g.A, g.lda): lda % 4 != 0
    run('f32', mode, 200, 136, 64, pa=3)
    # !ring_al16(g.B, g.ldb): ldb % 4 != 0
    run('f32', mode, 200, 136, 64, pb=5)
    # if (!a_km && (g.K & 3)) return -1: K % 4 != 0 (ragged K in the tile kernel's last slab), and K % 4 == 0 with a ragged last slab on the ring
    run('f32', mode, 130, 72, 66)
    run('f32', mode, 130, 72, 68)
    # K >= BK: K at 32 goes to the ring, K at 28 never asks it
    run('f32', mode, 70, 130, 32)
    run('f32', mode, 70, 130, 28)


def test_gemm_f32_ring_nn_n_and_bias_cap():
    # if (mode == 1 && g.b_idx) return -1: NN with a map on B's k rows goes to the tile kernel (load_km reads kidx); without it: ring
    run('f32', 1, 150, 136, 64, gather='b')
    run('f32', 1, 150, 136, 64, gather='ab')
    run('f32', 1, 150, 136, 64, gather='a')
    # if (g.k_chunk % RK != 0 || g.k_chunk <= 0) return -1 cannot be reached through the C ABI: every caller of sbr_gemm_ring_launch rounds
    # k_chunk up to a multiple of BK = RK = 32 (sbr_gemm_f32: ((K + BK - 1) / BK) * BK, BK for K = 0; sbr_gemm_nt_splitk_f32 and tn_slabs:
    # sbr_cdiv(..., BK) * BK of a positive count). Its far side, k_chunk a positive multiple of 32, is every ring case of this file.
    # if (b_kn && (g.N & 3)) return -1: N % 4 != 0 in NN falls back, N % 4 == 0 stays on the ring
    run('f32', 1, 150, 134, 64)
    run('f32', 1, 150, 136, 64)
    # if (mode != 2 && g.bias && g.N > RING_BIAS_CAP) return -1: a bias with N at 1024 (ring) and at 1028 (tile kernel); N = 1028 without bias: ring
    run('f32', 0, 70, 1024, 32, bias=True)
    run('f32', 0, 70, 1028, 32, bias=True)
    run('f32', 0, 70, 1028, 32)


@pytest.mark.parametrize('mode', (0, 1))
def test_gemm_f32_ring_big_items_switch(mode):
    # big_items >= 640: 639 items stay on the 64 x 128 ring tile, 640 take the 128 x 128 tile; ragged last panels on both
    run('f32', mode, 639 * 128 - 5, 128, 32, bias=mode == 0, act=1 if mode == 0 else 0)
    run('f32', mode, 639 * 128 + 3, 128, 32, bias=mode == 0, act=1 if mode == 0 else 0)
    # the 128 x 128 ring tile (ring_launch<2, ...>) over several slabs of the two-slot ring with a ragged last slab (K = 68: 3 slabs, K = 100:
    # 4 slabs, the last one 4 wide), two column panels with a ragged N, a ragged last row panel; with bias and an activation in NT
    run('f32', mode, 640 * 128 + 3, 136, 68, gather=True)
    run('f32', mode, 640 * 128 + 3, 136, 100, bias=mode == 0, act=2 if mode == 0 else 0, scatter=mode == 0)
    run('f32', mode, 320 * 128 + 77, 256, 132, bias=mode == 0, act=1 if mode == 0 else 0)
    # the 128 x 128 ring tile with more than one column panel, ragged N (n_left) and a scatter
    run('f32', mode, 80 * 128 + 7, 1000, 32, scatter=mode == 0)


@pytest.mark.parametrize('mode', (0, 1))
def test_gemm_f32_tile_kernel_shapes(mode):
    """the fallback tile kernel (reached with A 4 bytes off alignment): its three tile shapes and the XCD map"""
    # N <= 64: the 128 x 64 tile at N = 64, the 64 x 128 tile at N = 65
    run('f32', mode, 300, 64, 40, oa=1, bias=mode == 0, gather=True, scatter=mode == 0)
    run('f32', mode, 300, 65, 40, oa=1, bias=mode == 0, gather=True, scatter=mode == 0)
    # small_tile: sbr_cdiv(M, 128) * sbr_cdiv(N, 128) < 512 — 511 tiles (64 x 128 tile) and 512 tiles (128 x 128 tile)
    run('f32', mode, 511 * 128, 128, 36, oa=1, bias=mode == 0)
    run('f32', mode, 511 * 128 + 1, 128, 36, oa=1, bias=mode == 0)
    # g.xcd_map = g.mt >= 64: 63 row panels of the 64 x 128 tile (plain map) and 64 (XCD map), two column panels, ragged everywhere
    run('f32', mode, 63 * 64, 130, 36, oa=1)
    run('f32', mode, 63 * 64 + 1, 130, 36, oa=1)
    # g.xcd_map with mt not a multiple of 8 on the 128 x 64 tile (N <= 64), K % 4 != 0 and B off alignment as well
    run('f32', mode, 67 * 128 + 9, 60, 37, oa=1, ob=2)


@pytest.mark.parametrize('act', (0, 1, 2, 3, 4))
def test_gemm_f32_activations_gather_scatter(act):
    # every activation code on the ring (aligned) and on the tile kernel (!ring_al16(g.A, g.lda)); a_idx with heavy repeats, c_idx a partial
    # permutation of a larger C
    run('f32', 0, 100, 70, 48, act=act, bias=True, gather=True, scatter=True)
    run('f32', 0, 100, 70, 48, act=act, bias=True, gather=True, scatter=True, oa=1)
    run('f32', 0, 100, 70, 48, act=act, bias=False, oa=2)


@pytest.mark.parametrize('mode', (0, 1))
@pytest.mark.parametrize('act', (0, 1, 2, 3, 4))
@pytest.mark.parametrize('bias', (False, True))
def test_gemm_f32_k0_stores_act_of_bias(mode, act, bias):
    """K = 0 is an empty sum (include/sibrar_hip.h): modes 0 / 1 store act(bias), act(0) without a bias — exactly, except for the 2 ulp
    of a transcendental"""
    M, N = 70, 37
    Ab, Bb, Cb = _Buf(M, 4), _Buf(N, 4), _Buf(M, N, ld=N + 3, off=1)
    bias_t = R.gen_rand6((N,), 5) / 300 if bias else None
    call('sbr_gemm_f32', mode, Ab.ptr, Ab.ld, None, Bb.ptr, Bb.ld, None, _p(None if bias_t is None else bias_t.to(DEV)), Cb.ptr, Cb.ld, None,
         M, N, 0, act, 0, stream())
    got = Cb.check_untouched(what='K = 0')
    pre = (bias_t.double() if bias else torch.zeros(N, dtype=torch.float64))[None, :].expand(M, N)
    ref = R.ref_act(pre, act)
    R.check_bound(got, ref, R._act_bound(torch.zeros_like(ref), ref, pre, act), f'K = 0, mode {mode}, act {act}')
    if act in (0, 1):
        assert torch.equal(got.double(), ref)


# =================================================================================================================================
# sbr_gemm_f32, mode 2 (atomic accumulate)
# =================================================================================================================================
def test_gemm_f32_mode2_atomic():
    """sbr_gemm_f32 mode 2 never asks the ring: it always returns launch<2, 2, 1, 2, true, true> (the 64 x 128 tile kernel with float
    atomics), whatever the alignment, M % 4, N % 4, the maps or a bias. The conditions straddled here are the tile kernel's own."""
    # splits: max_splits = sbr_cdiv(K, 256) — K one below, at and above the boundary 256 (1, 1 and 2 K ranges)
    for K in (255, 256, 257):
        run('f32', 2, 96, 136, K)
    # load_km: c + 3 < nrows — whole 16-byte chunks along m / n (M % 4 == 0, N % 4 == 0) and a ragged last chunk on either operand, with maps
    # on both sides
    run('f32', 2, 97, 136, 600, gather=True)
    run('f32', 2, 96, 134, 600, gather=True)
    run('f32', 2, 96, 136, 600, gather=True)
    # g.vecA = aligned16(A, lda) / g.vecB = aligned16(B, ldb): operands off alignment (vecA / vecB = 0: the scalar loads of load_km)
    run('f32', 2, 70, 50, 300, oa=1, ob=3, gather=True)
    # a map on one side only (kidx ? kidx[gk] : gk in load_km and in the fast path): the other side must read the identity
    for g in ('a', 'b'):
        run('f32', 2, 96, 136, 600, gather=g)
        run('f32', 2, 97, 136, 600, gather=g)
    # if (g.bias && blockIdx.z == 0) v += g.bias[gn]: a bias in mode 2 is added once, by the first K range (3 ranges here); and without one
    run('f32', 2, 96, 136, 600, bias=True, gather='a')
    run('f32', 2, 96, 136, 600, bias=False, gather='a')


def test_gemm_f32_mode2_long_gathered_k_ranges():
    """Long gathered K ranges on the atomic tile kernel: 32 tiles want 32 K ranges, K = 32 * 512 gives k_chunk = 512 and K = 32 * 544 gives
    k_chunk = 544 (17 slabs per range, map entries far into a_idx / b_idx), with the maps on both sides and on each side alone. This is
    NOT the refusing side of the ring's `g.k_chunk > RING_IDX_CAP` lines: mode 2 of sbr_gemm_f32 never reaches sbr_gemm_ring_launch (see
    test_gemm_tn_ring_and_tile_kernel for why that side cannot be reached through the C ABI at all)."""
    run('f32', 2, 256, 1024, 32 * 512, gather=True, fams=('ints', 'rand6'))
    for g in (True, 'a', 'b'):
        run('f32', 2, 256, 1024, 32 * 544, gather=g, fams=('ints', 'rand6'))


def test_gemm_f32_mode2_k0_and_refusals():
    M, N = 70, 50
    Ab, Bb, Cb = _Buf(4, M), _Buf(4, N), _Buf(M, N, ld=N + 3, fill=7.0)
    # K == 0 (mode 2): an empty sum, nothing is launched and C keeps what it holds
    call('sbr_gemm_f32', 2, Ab.ptr, Ab.ld, None, Bb.ptr, Bb.ld, None, None, Cb.ptr, Cb.ld, None, M, N, 0, 0, 1, stream())
    assert bool((Cb.check_untouched(what='mode 2, K = 0') == 7.0).all())
    with pytest.raises(_err(), match='accumulate_atomic=1'):       # mode 2 without accumulate_atomic
        call('sbr_gemm_f32', 2, Ab.ptr, Ab.ld, None, Bb.ptr, Bb.ld, None, None, Cb.ptr, Cb.ld, None, M, N, 4, 0, 0, stream())
    with pytest.raises(_err(), match='activation with atomic accumulate'):
        call('sbr_gemm_f32', 2, Ab.ptr, Ab.ld, None, Bb.ptr, Bb.ld, None, None, Cb.ptr, Cb.ld, None, M, N, 4, 1, 1, stream())
    assert bool((Cb.check_untouched(what='refused calls') == 7.0).all())


# =================================================================================================================================
# sbr_gemm_nt_splitk_f32
# =================================================================================================================================
def test_gemm_nt_splitk_thresholds():
    ws = _lib().sbr_gemm_nt_splitk_workspace
    # tiles >= 96: 95 tiles of 64 x 128 are split, 96 are not (workspace query 0)
    assert ws(95 * 64, 128, 512) > 0 and ws(95 * 64 + 1, 128, 512) == 0
    run('nt_splitk', 0, 95 * 64, 128, 512, bias=True, act=1)
    # K < 8 * BK: K at 255 is not split, K at 256 is; max_splits = K / (4 * BK) clamps 48 wanted ranges to 2
    assert ws(256, 128, 255) == 0 and ws(256, 128, 256) == 2 * 256 * 128 * 4
    run('nt_splitk', 0, 256, 128, 256, bias=True, gather=True, scatter=True)
    # splits = 192 / tiles not clamped (64 tiles, 3 ranges of 16 allowed) and a ragged K (k_chunk rounds up to whole slabs)
    assert ws(4096, 128, 2048) == 3 * 4096 * 128 * 4
    run('nt_splitk', 0, 4096, 128, 2048)
    run('nt_splitk', 0, 1408, 128, 772, bias=True, act=2, gather=True, scatter=True)
    # the tile kernel behind the same entry: !ring_al16(g.A, g.lda) (A 4 bytes off), K % 4 != 0, and N ragged
    run('nt_splitk', 0, 300, 100, 772, bias=True, act=4, gather=True, scatter=True, oa=1)
    run('nt_splitk', 0, 300, 100, 771, bias=True, act=3)


def test_gemm_nt_splitk_refusals():
    M, N, K = 256, 128, 512
    Ab, Bb, Cb = _Buf(M, K), _Buf(N, K), _Buf(M, N, ld=N + 3)
    need = _lib().sbr_gemm_nt_splitk_workspace(M, N, K)
    wsb = _ws(need)
    with pytest.raises(_err(), match='workspace too small'):       # one byte short
        call('sbr_gemm_nt_splitk_f32', Ab.ptr, Ab.ld, None, Bb.ptr, Bb.ld, None, Cb.ptr, Cb.ld, None, M, N, K, 0, wsb.ptr, need - 1, stream())
    with pytest.raises(_err(), match='is not split'):              # a shape whose workspace query returns 0
        call('sbr_gemm_nt_splitk_f32', Ab.ptr, Ab.ld, None, Bb.ptr, Bb.ld, None, Cb.ptr, Cb.ld, None, M, N, 255, 0, wsb.ptr, need, stream())
    Cb.check_untouched(written_rows=[], what='refused nt_splitk')
    wsb.check_untouched(written_rows=[], what='refused nt_splitk workspace')


# =================================================================================================================================
# sbr_gemm_tn_f32, sbr_gemm_tn_f32_slabs, sbr_splitk_reduce_multi(_fin)
# =================================================================================================================================
def test_gemm_tn_ring_and_tile_kernel():
    """tn_slabs (behind sbr_gemm_tn_f32 and sbr_gemm_tn_f32_slabs) is the ONLY caller of sbr_gemm_ring_launch with mode 2. Three of the
    ring's eligibility lines therefore have a side that cannot be reached through the C ABI:
      * if (a_km && g.a_idx && g.k_chunk > RING_IDX_CAP) return -1 and the same line for b_idx: tn_splits raises the split count to
        min_splits = sbr_cdiv(K, 512), so sbr_cdiv(K, splits) <= 512 and k_chunk, its round-up to whole slabs of 32, is at most 512 =
        RING_IDX_CAP. The passing side AT the cap is the 444 x 128 x 74 * 512 cases below;
      * if (mode == 2 && g.bias) return -1: tn_slabs sets g.bias = nullptr (the TN entries take no bias); every ring case below is its
        passing side.
    sbr_gemm_f32 mode 2 does take maps, long K ranges and a bias, but it always runs the atomic tile kernel (test_gemm_f32_mode2_atomic)."""
    # ring: M % 4 == 0 and N % 4 == 0; if (a_km && (g.M & 3)) return -1; if (b_kn && (g.N & 3)) return -1
    run('tn', 2, 96, 136, 1000, gather=True, expect_split=0)
    run('tn', 2, 97, 136, 1000, gather=True, expect_split=0)
    run('tn', 2, 96, 134, 1000, gather=True, expect_split=0)
    run('tn', 2, 96, 136, 1000, expect_split=0)
    # a map on one side only, on the ring and on the tile kernel
    for g in ('a', 'b'):
        run('tn', 2, 96, 136, 1000, gather=g, expect_split=0)
        run('tn', 2, 97, 134, 1000, gather=g, expect_split=0)
    # K >= BK: K = 20 goes straight to the tile kernel; a single slab
    run('tn', 2, 64, 128, 20, expect_split=0)
    # g.k_chunk > RING_IDX_CAP, passing side at the cap: 7 tiles want 74 ranges, K = 74 * 512 puts k_chunk AT 512 staged k-row indices, with
    # both maps (the a_idx line and the b_idx line), and with b_idx alone
    run('tn', 2, 444, 128, 74 * 512, gather=True, fams=('ints', 'rand6'), expect_split=0)
    run('tn', 2, 444, 128, 74 * 512, gather='b', fams=('ints', 'rand6'), expect_split=0)


def test_gemm_tn_split_kernel_against_ring(monkeypatch):
    monkeypatch.delenv('SBR_GEMM_SPLIT', raising=False)
    monkeypatch.delenv('SBR_TN_SPLIT', raising=False)
    # sbr_tn_split_splits: M % 128 != 0 / N % 128 != 0 / K < 4096 stay on the fp32 ring, 128 x 128 x 4096 goes to the bf16-split kernel
    run('tn_split', 2, 128, 128, 4096, gather=True, expect_split=1)
    run('tn_split', 2, 128, 256, 4096 + 37, expect_split=1)              # nj * nm > 1: the WIDE instantiation, ragged last chunk
    run('tn_split', 2, 128, 128, 4096 + 5, gather='a', expect_split=1)     # a map on one side only: the other side reads the identity
    run('tn_split', 2, 256, 128, 4096, gather='b', expect_split=1)
    run('tn', 2, 128, 128, 4095, gather=True, expect_split=0)
    run('tn', 2, 132, 128, 4096, expect_split=0)
    run('tn', 2, 128, 132, 4096, expect_split=0)
    # sbr_tn_split_launch: lda % 2 != 0 and A 4 bytes off alignment return -1 (and the ring refuses them too: tile kernel). The split
    # bound is not claimed here: these run on the fp32 pipe
    run('tn', 2, 128, 128, 4096, pa=3, expect_split=1)
    run('tn', 2, 128, 128, 4096, oa=1, gather=True, expect_split=1)
    # tn_slabs: (long)ss * M * N * sizeof(float) <= workspace_bytes fails — a workspace that fits tn_splits (32 slabs) but not the split kernel's
    # 128: the fp32 ring serves the call
    assert _tn_splits(128, 128, 4096) == 32 and _lib().sbr_gemm_tn_f32_workspace(128, 128, 4096) == 128 * 128 * 128 * 4
    run('tn', 2, 128, 128, 4096, ws_bytes=32 * 128 * 128 * 4, expect_split=1)
    # SBR_TN_SPLIT=0: read per call; the query and the launch both answer "ring"
    monkeypatch.setenv('SBR_TN_SPLIT', '0')
    run('tn', 2, 128, 128, 4096, gather=True, expect_split=0)
    monkeypatch.delenv('SBR_TN_SPLIT')
    assert _lib().sbr_gemm_tn_split_supported(128, 128, 4096) == 1


def test_gemm_tn_longest_reduction():
    # 128 x 128 x 600,000: the longest reduction the exactness claim of the ints family is asserted for (test_gemm_refs_cpu.py)
    run('tn_split', 2, 128, 128, R.K_MAX_GPU, fams=('ints', 'rand6'), expect_split=1)


def test_gemm_tn_k0_and_workspace_refusal():
    M, N = 70, 50
    Ab, Bb, Cb = _Buf(4, M), _Buf(4, N), _Buf(M, N, ld=N + 3)
    need = _lib().sbr_gemm_tn_f32_workspace(M, N, 0)
    assert need == M * N * 4
    wsb = _ws(need)
    call('sbr_gemm_tn_f32', Ab.ptr, Ab.ld, None, Bb.ptr, Bb.ld, None, Cb.ptr, Cb.ld, M, N, 0, wsb.ptr, need, stream())     # K = 0: all zeros
    assert bool((Cb.check_untouched(what='tn K = 0') == 0).all())
    wsb.check_untouched(what='tn K = 0 workspace')
    need = M * N * 4 * _tn_splits(M, N, 300)
    Cb2 = _Buf(M, N, ld=N + 3)
    Ab2, Bb2 = _Buf(300, M), _Buf(300, N)
    with pytest.raises(_err(), match='workspace too small'):
        call('sbr_gemm_tn_f32', Ab2.ptr, Ab2.ld, None, Bb2.ptr, Bb2.ld, None, Cb2.ptr, Cb2.ld, M, N, 300, _ws(need).ptr, need - 1, stream())
    Cb2.check_untouched(written_rows=[], what='refused tn')


def _arr(ct, vals):
    return ctypes.cast((ct * len(vals))(*vals), ctypes.c_void_p)


@pytest.mark.parametrize('shapes', (((96, 136, 700),), ((96, 134, 700), (33, 7, 100)), ((128, 128, 4096), (96, 136, 700))))
def test_splitk_reduce_multi_with_padded_outputs(shapes):
    """sbr_gemm_tn_f32_slabs + sbr_splitk_reduce_multi through the C ABI with ldc > N: the float4 reducer (every N % 4 == 0: ldc = N + 4
    keeps the rows aligned, ldc = N + 3 takes its scalar stores) and the scalar reducer (an N % 4 != 0 among the products)"""
    for pc in (4, 3):
        for fam in ('ints', 'rand6'):
            prods = []
            for q, (M, N, K) in enumerate(shapes):
                a, b = R.family(fam, (K, M), 0, (K, N), 0, 11 * q)
                Ab, Bb = _Buf(K, M, ld=M + 4, data=a), _Buf(K, N, ld=N + 4, data=b)
                need = _lib().sbr_gemm_tn_f32_workspace(M, N, K)
                wsb, Cb = _ws(need), _Buf(M, N, ld=N + pc)
                splits = ctypes.c_int(0)
                call('sbr_gemm_tn_f32_slabs', Ab.ptr, Ab.ld, None, Bb.ptr, Bb.ld, None, M, N, K, wsb.ptr, need,
                     ctypes.cast(ctypes.pointer(splits), ctypes.c_void_p), stream())
                assert 1 <= splits.value and splits.value * M * N * 4 <= need
                wsb.check_untouched(what='slabs workspace')
                prods.append((Ab, Bb, wsb, Cb, M, N, K, splits.value))
            args = (len(prods), _arr(ctypes.c_void_p, [p[2].ptr for p in prods]), _arr(ctypes.c_void_p, [p[3].ptr for p in prods]),
                    _arr(ctypes.c_long, [p[3].ld for p in prods]), _arr(ctypes.c_int, [p[4] for p in prods]),
                    _arr(ctypes.c_int, [p[5] for p in prods]), _arr(ctypes.c_int, [p[7] for p in prods]))
            outs = []
            for rep in range(2):
                call('sbr_splitk_reduce_multi', *args, stream())
                outs.append([p[3].check_untouched(what=f'reduce_multi ldc = N + {pc}').clone() for p in prods])
            for q, (Ab, Bb, wsb, Cb, M, N, K, sp) in enumerate(prods):
                ref, pre, Sm = R.ref_tn(_flat(Ab), Ab.ld, None, _flat(Bb), Bb.ld, None, M, N, K)
                split = bool(_lib().sbr_gemm_tn_split_supported(M, N, K))
                what = f'slabs + reduce_multi {M}x{N}x{K} [{fam}]'
                if fam == 'ints':
                    R.check_exact(outs[0][q], ref, what)
                else:
                    r = R.check_bound(outs[0][q], ref, (R.bound_split if split else R.bound_f32)(Sm, K), what)
                    RATIOS['sbr_splitk_reduce_multi'] = max(RATIOS.get('sbr_splitk_reduce_multi', 0.0), r)
                _assert_bits(outs[1][q], outs[0][q], what + ' second reduction')


@pytest.mark.parametrize('count', (1, 8, 9))
def test_deferred_tn_pending_products(count):
    """1, 8 and 9 pending products through ops.DeferredTN: the ninth takes a second sbr_splitk_reduce_multi launch; one finish() also
    takes a pending column sum along (sbr_splitk_reduce_multi_fin) when at most 8 products are pending"""
    ops = S().ops
    d = ops.DeferredTN()
    keep = []
    for q in range(count):
        M, N, K = (128, 128, 4096) if q == 0 else (32 + 4 * q, 64 + 8 * q, 200 + 31 * q)
        a, b = R.family('ints' if q % 2 else 'rand6', (K, M), 0, (K, N), 0, q)
        out = torch.full((M, N), float('nan'), device=DEV)
        d.matmul_tn(q, a.to(DEV), b.to(DEV), out=out)
        keep.append((a, b, out, M, N, K, q % 2 == 1))
    x = R.gen_ints((500, 64), 3).to(DEV)
    cs_out = torch.full((64,), float('nan'), device=DEV)
    ws = torch.zeros(17 * 64, device=DEV, dtype=torch.float64)
    ws.view(17, 64)[3] = x.double().sum(0)                                  # a pending column sum in one replica
    took = d.finish(colred=[(ws, cs_out)])
    torch.cuda.synchronize()
    assert took == (count <= 8)
    if took:
        assert torch.equal(cs_out.cpu().double(), x.double().sum(0).cpu()) and not bool(ws.view(17, 64)[1:].any())
    for a, b, out, M, N, K, exact in keep:
        ref, _, Sm = R.ref_tn(a.reshape(-1), M, None, b.reshape(-1), N, None, M, N, K)
        if exact:
            R.check_exact(out.cpu(), ref, f'DeferredTN {M}x{N}x{K}')
        else:
            split = bool(_lib().sbr_gemm_tn_split_supported(M, N, K))
            R.check_bound(out.cpu(), ref, (R.bound_split if split else R.bound_f32)(Sm, K), f'DeferredTN {M}x{N}x{K}')


# =================================================================================================================================
# sbr_gemm_wres_f32 and sbr_gemm_split_f32 (N = K = 128)
# =================================================================================================================================
M_EDGES = (1, 31, 32, 33, 63, 64, 65)


@pytest.mark.parametrize('entry', ('wres', 'split'))
@pytest.mark.parametrize('mode', (0, 1))
def test_wres_split_row_counts(entry, mode):
    # M around the 32-row blocks (split: one wave per block) and the 64-row tiles (wres: WR_BM); C 4 bytes off alignment with an odd ldc: the
    # stores are one float per lane and need no alignment (include/sibrar_hip.h); lda, ldw, ldc each larger than 128
    for i, M in enumerate(M_EDGES):
        run(entry, mode, M, 128, 128, bias=mode == 0, act=(1, 2, 0, 4, 3, 1, 0)[i] if mode == 0 else 0, pa=4, pb=8, pc=3, oc=1)
    # every workgroup more than one block / tile: wres runs at most 512 workgroups of 64-row tiles, split at most 256 x 8 waves of 32-row blocks
    big = 512 * 64 + 64 + 5 if entry == 'wres' else 256 * 8 * 32 + 32 + 7
    run(entry, mode, big, 128, 128, bias=mode == 0, act=1 if mode == 0 else 0)
    # the shape of the training step
    run(entry, mode, 90112, 128, 128, bias=mode == 0, act=1 if mode == 0 else 0, fams=('ints', 'rand6'))


@pytest.mark.parametrize('entry', ('wres', 'split'))
@pytest.mark.parametrize('act', (1, 2))
def test_wres_split_y_epilogue_and_colsum(entry, act):
    """mode 1 with Y: C = (A W) * act'(Y) and the pending column sums of C in the replica layout (17 x 128 doubles)"""
    name = f'sbr_gemm_{entry}_f32'
    for M in (33, 65, 5000):
        for fam in ('ints', 'rand6'):
            a, w = R.family(fam, (M, 128), 1, (128, 128), 0, M)
            y = R.ref_act(torch.randn(M, 128, generator=torch.Generator().manual_seed(M)).double(), act).float()
            Ab, Wb, Yb = _Buf(M, 128, ld=132, data=a), _Buf(128, 128, ld=136, data=w), _Buf(M, 128, ld=131, off=1, data=y)
            Cb = _Buf(M, 128, ld=133, off=1)
            ws = torch.zeros(17 * 128, device=DEV, dtype=torch.float64)
            call(name, 1, Ab.ptr, Ab.ld, Wb.ptr, Wb.ld, None, Cb.ptr, Cb.ld, M, 128, 128, act, Yb.ptr, Yb.ld, ws.data_ptr(), stream())
            got = Cb.check_untouched(what=name + ' Y epilogue')
            prod, _, Sm = R.ref_nn(_flat(Ab), Ab.ld, None, _flat(Wb), Wb.ld, M, 128, 128)
            g = ref_act_grad_from_out(y.double(), act)
            ref = prod * g
            pb = (R.bound_split if entry == 'split' else R.bound_f32)(Sm, 128)
            bound = pb * g.abs() + prod.abs() * act_grad_err(y.double(), act) + R.U32 * ref.abs() + 1e-300
            what = f'{name} Y epilogue act {act} M {M} [{fam}]'
            if fam == 'ints' and act == 1:
                R.check_exact(got, ref, what)
            else:
                R.check_bound(got, ref, bound, what)
            # column sums: fp32 partial sums of at most 16 of the stored values, then double atomics
            assert not bool(ws[:128].any()), 'the totals row belongs to sbr_colred_finish'
            cs = ws.view(17, 128)[1:].sum(0).cpu()
            cref = got.double().sum(0)
            cb = R.gamma(16) * got.double().abs().sum(0) + 1e-12 * got.double().abs().sum(0)
            R.check_bound(cs, cref, cb, what + ' column sums')
            if fam == 'ints' and act == 1:
                assert torch.equal(cs, cref)


@pytest.mark.parametrize('entry', ('wres', 'split'))
def test_wres_split_refusals(entry):
    name = f'sbr_gemm_{entry}_f32'
    M = 40
    Cb = _Buf(M, 128, ld=131)
    Yb = _Buf(M, 128, fill=0.5)
    bias = torch.zeros(128, device=DEV)

    def go(mode, Ab, Wb, bias_d=None, Y=None):
        call(name, mode, Ab.ptr, Ab.ld, Wb.ptr, Wb.ld, _p(bias_d), Cb.ptr, Cb.ld, M, 128, 128, 0, _p(Y), 128 if Y is not None else 0, None, stream())

    ok_a, ok_w = _Buf(M, 128, ld=132, fill=1.0), _Buf(128, 128, ld=132, fill=1.0)
    for mode in (0, 1):
        with pytest.raises(_err(), match='16-byte aligned'):       # A 4 bytes off / lda % 4 != 0
            go(mode, _Buf(M, 128, ld=132, off=1, fill=1.0), ok_w)
        with pytest.raises(_err(), match='16-byte aligned'):
            go(mode, _Buf(M, 128, ld=131, fill=1.0), ok_w)
    with pytest.raises(_err(), match='16-byte aligned'):           # W misaligned in mode 0 (16-byte loads of its rows)
        go(0, ok_a, _Buf(128, 128, ld=132, off=1, fill=1.0))
    with pytest.raises(_err(), match='mode 1 without bias'):       # Y in mode 0
        go(0, ok_a, ok_w, Y=Yb.t)
    with pytest.raises(_err(), match='mode 1 without bias'):       # Y with a bias
        go(1, ok_a, ok_w, bias_d=bias, Y=Yb.t)
    with pytest.raises(_err(), match='not supported'):
        call(name, 0, ok_a.ptr, ok_a.ld, ok_w.ptr, ok_w.ld, None, Cb.ptr, Cb.ld, M, 128, 96, 0, None, 0, None, stream())
    Cb.check_untouched(written_rows=[], what='refused ' + name)
    lib = _lib()
    sup = getattr(lib, f'sbr_gemm_{entry}_supported')
    assert sup(1, 128, 128) == 1 and sup(0, 128, 128) == 0 and sup(5, 127, 128) == 0 and sup(5, 128, 160) == 0
    if entry == 'split':
        # mode 1 reads W one float per lane (mode == 1 || sp_al16(W, ldw)): a W 4 bytes off alignment with an odd ldw works
        run('split', 1, 70, 128, 128, ob=1, pb=3)
    else:
        with pytest.raises(_err(), match='16-byte aligned'):       # wres loads W through 16-byte reads / k-quads in both modes
            go(1, ok_a, _Buf(128, 128, ld=132, off=1, fill=1.0))


# =================================================================================================================================
# sbr_gemm_split_proj_f32 and sbr_gemm_split_wide_f32
# =================================================================================================================================
def test_split_proj():
    sup = _lib().sbr_gemm_split_proj_supported
    # M >= 1 && N == SP_N && K >= 2 * SP_K && K % PJ_KC == 0, both sides of every term
    assert [sup(1, 128, 256), sup(0, 128, 256), sup(5, 127, 256), sup(5, 129, 256), sup(5, 128, 192), sup(5, 128, 288), sup(5, 128, 320)] == \
        [1, 0, 0, 0, 0, 0, 1]
    # gather + scatter with guards on C, ragged last 32-row block, ldw > K, every activation; C 4 bytes off alignment with an odd ldc
    for i, (M, K) in enumerate(((1, 256), (33, 320), (95, 768), (1408, 768), (45056 // 8 + 3, 256))):
        run('proj', 0, M, 128, K, gather=True, scatter=True, bias=True, act=(0, 1, 2, 3, 4)[i], pb=8, pc=3, oc=1)
    run('proj', 0, 64, 128, 512)
    # more blocks than the grid's waves take in one pass (256 workgroups x 8 waves x 32 rows)
    run('proj', 0, 256 * 8 * 32 + 45, 128, 256, gather=True, bias=True, act=1, fams=('ints', 'rand6'))
    # half-item mode of the last round, rem > S && 2 * rem <= 3 * S at the capped grid (256 workgroups: S = 1,024 blocks of 32 rows, one
    # round = 2 S): both sides of each term — rem = 1,024 (rem > S fails), 1,025 and 1,536 (both hold), 1,537 (2 * rem <= 3 * S fails);
    # every last block is ragged
    for blocks in (1024, 1025, 1536, 1537):
        run('proj', 0, 32 * blocks - 3, 128, 256, gather=True, bias=True, act=1, fams=('ints', 'rand6'))
    M = 40
    Ab, Wb, Cb = _Buf(M, 256, ld=260, fill=1.0), _Buf(128, 256, ld=260, fill=1.0), _Buf(M, 128, ld=131)
    for A, W in ((_Buf(M, 256, ld=260, off=1, fill=1.0), Wb), (_Buf(M, 256, ld=259, fill=1.0), Wb), (Ab, _Buf(128, 256, ld=260, off=2, fill=1.0))):
        with pytest.raises(_err(), match='16-byte aligned'):
            call('sbr_gemm_split_proj_f32', A.ptr, A.ld, None, W.ptr, W.ld, None, Cb.ptr, Cb.ld, None, M, 128, 256, 0, stream())
    with pytest.raises(_err(), match='not supported'):
        call('sbr_gemm_split_proj_f32', Ab.ptr, Ab.ld, None, Wb.ptr, Wb.ld, None, Cb.ptr, Cb.ld, None, M, 128, 192, 0, stream())
    Cb.check_untouched(written_rows=[], what='refused proj')


@pytest.mark.parametrize('mode', (0, 1))
def test_split_wide(mode):
    sup = _lib().sbr_gemm_split_wide_supported
    # M >= 1 && N >= SW_N && N % SW_N == 0 && K >= 2 * SW_KC && K % SW_KC == 0, both sides of every term
    assert [sup(1, 256, 64), sup(0, 256, 64), sup(5, 0, 64), sup(5, 128, 64), sup(5, 384, 64), sup(5, 512, 64), sup(5, 256, 32), sup(5, 256, 80),
            sup(5, 256, 96)] == [1, 0, 0, 0, 0, 1, 0, 0, 1]
    # NT with bias and activation, NN without bias (the input gradient); gather and scatter; ragged last block; ldw > the row
    for i, (M, N, K) in enumerate(((1, 256, 64), (33, 256, 96), (257, 512, 128), (300, 256, 512), (2500, 512, 256))):
        run('wide', mode, M, N, K, gather=True, scatter=True, bias=mode == 0, act=(1, 2, 3, 4, 0)[i] if mode == 0 else 0, pb=8, pc=3, oc=1)
    # the largest shape kept: 30,805 x 512 x 1,024 (more row groups than the 256 workgroups take in one pass)
    run('wide', mode, 30805, 512, 1024, bias=mode == 0, act=1 if mode == 0 else 0, fams=('ints', 'rand6'))
    M = 40
    Ab, Cb = _Buf(M, 64, ld=68, fill=1.0), _Buf(M, 256, ld=259)
    Wb = _Buf(256, 64, ld=68, fill=1.0) if mode == 0 else _Buf(64, 256, ld=260, fill=1.0)
    with pytest.raises(_err(), match='16-byte aligned'):
        A = _Buf(M, 64, ld=68, off=1, fill=1.0)
        call('sbr_gemm_split_wide_f32', mode, A.ptr, A.ld, None, Wb.ptr, Wb.ld, None, Cb.ptr, Cb.ld, None, M, 256, 64, 0, stream())
    if mode == 0:
        with pytest.raises(_err(), match='16-byte aligned'):       # mode == 1 || sp_al16(W, ldw)
            W = _Buf(256, 64, ld=67, fill=1.0)
            call('sbr_gemm_split_wide_f32', 0, Ab.ptr, Ab.ld, None, W.ptr, W.ld, None, Cb.ptr, Cb.ld, None, M, 256, 64, 0, stream())
    else:
        run('wide', 1, 70, 256, 64, ob=1, pb=3)                    # NN reads W one float per lane: any base and ldw
    with pytest.raises(_err(), match='not supported'):
        call('sbr_gemm_split_wide_f32', mode, Ab.ptr, Ab.ld, None, Wb.ptr, Wb.ld, None, Cb.ptr, Cb.ld, None, M, 128, 64, 0, stream())
    Cb.check_untouched(written_rows=[], what='refused wide')


def test_zz_report_ratios():
    """the largest err / bound per entry point on the random family (run with -s to read it); every figure is <= 1 by the asserts above"""
    print('GEMM_RATIOS ' + json.dumps({k: round(v, 4) for k, v in sorted(RATIOS.items())}))
    assert all(v <= 1.0 for v in RATIOS.values())
