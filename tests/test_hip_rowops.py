"""GPU: the row-wise kernels (csrc/rowops.hip) and the two cast kernels of the scorers, each C entry point on both sides of every
dispatch condition of its host function, against plain float64 torch-CPU references written here from the operation's definition.

Conventions of this file
  * u = 2^-24 is the unit roundoff of fp32. An fp32 sum of m terms, in ANY order, has |err| <= (m - 1) u sum|terms| to first order
    (each of the m - 1 additions rounds once, relative to a partial sum that is at most sum|terms|); the tests assert
    m u sum|terms|, evaluated per output element in float64. Bounds are derived from the kernels' arithmetic, never fitted.
  * Operands are views into larger flat buffers pre-filled with NaN (``_Buf``): a row stride larger than the row, a base pointer
    4 or 8 bytes off a 16-byte boundary (so the scalar fallback runs at a D that would otherwise vectorise), and guard elements
    in front, behind and between the rows. After every call the test asserts that every element outside the addressed rows and
    columns still is NaN (a tail that writes past n or past D), and a read past a row would poison the result with NaN.
  * Row counts: 1, one below / at / one above the block or wave quantum of the kernel, and one count that makes a capped grid run
    its grid-stride loop twice (the caps are 4,096 blocks of 256 threads = 1,048,576 elements; 2,048 blocks x 16 rows for the
    D = 128 scatter-add; 8,192 blocks for the casts)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from hip_testutil import (DEV, GUARD, NAN, U32, S, _L, _assert_bits, _assert_bound, _bits, _Buf, _dev, _i32, _i64, _orders, _p, _rand, _ulp,
                          call, stream)

pytestmark = pytest.mark.gpu
DS = [1, 3, 4, 12, 16, 24, 64, 68, 96, 100, 128, 130, 256, 260, 300]


# ---------------------------------------------------------------------------------------------------------------------------------
# lookup: sbr_gather_rows / LookupFn forward, sbr_lookup_rows, sbr_resolve_rows
# ---------------------------------------------------------------------------------------------------------------------------------
def _gather_cases():
    cases = []
    for D in DS:
        cases.append((5, D, 0, 0, 0, 0, False))                                   # dense, aligned: float4 path iff D % 4 == 0
        cases.append((257, D, 4, 8, 0, 0, True))                                  # strides that keep multiples of 4, out_idx
        if D % 4 == 0:
            cases.append((64, D, 0, 0, 1, 0, False))                              # W 4 bytes off -> scalar
            cases.append((65, D, 0, 0, 0, 2, True))                               # out 8 bytes off -> scalar
            cases.append((63, D, 1, 0, 0, 0, False))                              # ldw % 4 != 0 -> scalar
            cases.append((1, D, 0, 2, 0, 0, True))                                # ldo % 4 != 0 -> scalar
    cases.append((349_600, 3, 0, 0, 0, 0, False))                                 # scalar kernel, 1,048,800 elements: second trip of the capped grid
    cases.append((262_200, 4, 0, 0, 1, 0, True))                                  # the same through the misaligned fallback at D = 4
    cases.append((262_200, 4, 0, 0, 0, 0, False))                                 # float4 kernel above 1,048,576 elements (no cap: one thread per quad)
    return cases


@pytest.mark.parametrize('n,D,xw,xo,off_w,off_o,use_oi', _gather_cases())
def test_gather_rows(n, D, xw, xo, off_w, off_o, use_oi):
    """out[oi(j), :] = W[rows[j], :] bit for bit (a copy: no arithmetic). float4 kernel iff D, ldw, ldo are multiples of 4 and both base
    pointers are 16-byte aligned; each case names the condition it breaks. rows repeat heavily (n_table << n)."""
    n_table = 37
    W = _Buf(n_table, D, D + xw, off_w, data=_rand(n_table, D, seed=D))
    n_out = n + 3 if use_oi else n
    out = _Buf(n_out, D, D + xo, off_o)
    rng = np.random.default_rng(n + D)
    rows = rng.integers(0, n_table, size=n)
    oi = rng.permutation(n_out)[:n] if use_oi else None
    rows_d, oi_d = _i32(rows), (_i32(oi) if use_oi else None)
    call('sbr_gather_rows', W.ptr, W.ld, _p(rows_d), out.ptr, out.ld, _p(oi_d), n, D, stream())
    dst = torch.as_tensor(oi if use_oi else np.arange(n))
    got = out.check_untouched(dst, 'gather_rows')
    _assert_bits(got[dst], W.host()[torch.as_tensor(rows)], 'gather_rows')


@pytest.mark.parametrize('D', [3, 64, 130])
def test_lookup_fn_forward_and_backward(D):
    """ops.LookupFn: forward == indexing bit for bit; backward == index_add_ in float64 within m u sum|terms| (m sources of a table row:
    m - 1 atomic additions into a zeroed gradient, any order)."""
    ops = S().ops
    n_table = 50
    W = _rand(n_table, D, seed=1)
    idx = torch.from_numpy(np.random.default_rng(D).integers(0, n_table, size=(70, 5)))
    idx[:, 0] = 7                                                                  # one hot row
    Wd = W.to(DEV).requires_grad_(True)
    y = ops.LookupFn.apply(Wd, idx.to(DEV))
    assert y.shape == (70, 5, D)
    _assert_bits(y.detach().cpu(), W[idx], 'LookupFn fwd')
    g = _rand(70, 5, D, seed=2)
    (y * g.to(DEV)).sum().backward()
    ref = torch.zeros(n_table, D, dtype=torch.float64).index_add_(0, idx.reshape(-1), g.reshape(-1, D).double())
    mag = torch.zeros(n_table, D, dtype=torch.float64).index_add_(0, idx.reshape(-1), g.reshape(-1, D).double().abs())
    m = torch.bincount(idx.reshape(-1), minlength=n_table).double()[:, None]
    _assert_bound(Wd.grad.cpu(), ref, m * U32 * mag, 'LookupFn bwd')


def test_lookup_rows_supported_reports_each_condition():
    lib = _L().lib()
    base = torch.zeros(4096, device=DEV)
    a = base.data_ptr()
    assert a % 16 == 0
    ok = lambda W, ldw, out, ldo, D: int(lib.sbr_lookup_rows_supported(W, ldw, out, ldo, D))
    assert ok(a, 64, a + 1024, 64, 64) == 1 and ok(a, 8, a + 1024, 4, 4) == 1
    assert ok(a, 64, a + 1024, 64, 0) == 0 and ok(a, 3, a + 1024, 3, 3) == 0 and ok(a, 66, a + 1024, 66, 66) == 0       # D
    assert ok(a, 65, a + 1024, 64, 64) == 0 and ok(a, 64, a + 1024, 66, 64) == 0                                         # strides
    assert ok(a + 4, 64, a + 1024, 64, 64) == 0 and ok(a, 64, a + 1032, 64, 64) == 0                                     # base pointers


@pytest.mark.parametrize('n,D,xw,xo,use_map', [(1, 4, 0, 0, False), (63, 16, 4, 0, True), (64, 16, 0, 4, False), (65, 128, 8, 8, True),
                                               (1000, 12, 0, 4, True), (3, 300, 0, 0, True), (5000, 260, 0, 0, False), (17, 68, 4, 0, True)])
def test_lookup_rows(n, D, xw, xo, use_map):
    """sbr_lookup_rows: out[j] = W[row(idx[j])], rows_out[j] = row(idx[j]) with row = rowmap[id] (or id); ids that are negative, past the
    map or mapped to -1 set the flag and read row 0. Bit-exact. A layout the entry does not take is refused with a clean error."""
    n_table, n_ids = 29, 41
    rng = np.random.default_rng(n * D)
    W = _Buf(n_table, D, D + xw, 0, data=_rand(n_table, D, seed=3))
    out = _Buf(n, D, D + xo, 0)
    rowmap = rng.permutation(n_ids).astype(np.int64)
    rowmap[rowmap >= n_table] = -1                                                 # ids without a row in this split
    map_len = n_ids if use_map else n_table
    for with_missing in (False, True):
        valid = np.flatnonzero(rowmap >= 0) if use_map else np.arange(n_table)
        ids = rng.choice(valid, size=n)
        if with_missing:
            bad = [-1, map_len, map_len + 5] + ([int(np.flatnonzero(rowmap < 0)[0])] if use_map else [])
            for q, b in enumerate(bad):
                ids[(q * 7) % n] = b
        want = np.array([(rowmap[i] if use_map else i) if 0 <= i < map_len else -1 for i in ids])
        missing = want < 0
        want[missing] = 0
        out.flat.fill_(NAN)
        ids_d, map_d = _i64(ids), (_i32(rowmap) if use_map else None)
        rows_out = torch.full((n + 8,), -7, dtype=torch.int32, device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        call('sbr_lookup_rows', _p(ids_d), n, _p(map_d), map_len, W.ptr, W.ld, _p(rows_out), out.ptr, out.ld, D, _p(err), stream())
        assert int(err) == int(missing.any())
        assert rows_out[:n].cpu().tolist() == want.tolist() and rows_out[n:].cpu().tolist() == [-7] * 8
        got = out.check_untouched(None, 'lookup_rows')
        _assert_bits(got, W.host()[torch.as_tensor(want)], 'lookup_rows')
    # unsupported layouts: a clean error, nothing launched
    Wm = _Buf(n_table, D, D + xw, 1, fill=0.0)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(_L().SibrarHipError):
        call('sbr_lookup_rows', _p(ids_d), n, None, n_table, Wm.ptr, Wm.ld, _p(rows_out), out.ptr, out.ld, D, _p(err), stream())


@pytest.mark.parametrize('n,k', [(1, 1), (255, 3), (256, 1), (257, 2), (5000, 3)])
def test_resolve_rows(n, k):
    """rows[j] = map_seg(j)[idx[slots[j] / k]] over three segments (an identity map, a map with holes, a short map); ids outside a
    segment's map or mapped to -1 give row 0 and set the flag. Exact."""
    rng = np.random.default_rng(n + k)
    n_idx = 90
    idx = rng.integers(0, 60, size=n_idx).astype(np.int64)
    offs = np.array([0, n // 3, n // 3 + n // 4, n], dtype=np.int32)
    map1 = rng.permutation(60).astype(np.int32)
    map1[::9] = -1
    map2 = rng.permutation(40).astype(np.int32)                                     # ids 40 .. 59 are past this map
    maps = [None, map1, map2]
    lens = np.array([50, 60, 40], dtype=np.int32)                                   # segment 0: identity over 50 rows (ids 50 .. 59 are missing)
    slots = rng.integers(0, n_idx * k, size=n).astype(np.int32)
    for with_missing in (True, False):
        if not with_missing:
            idx = rng.integers(0, 40, size=n_idx).astype(np.int64)
            map1 = np.abs(map1)
            maps[1] = map1
        want, miss = np.zeros(n, dtype=np.int64), False
        for j in range(n):
            s = int(np.searchsorted(offs[1:], j, side='right'))
            i = idx[slots[j] // k]
            r = -1 if not (0 <= i < lens[s]) else (int(maps[s][i]) if maps[s] is not None else int(i))
            miss |= r < 0
            want[j] = max(r, 0)
        dmaps = [None if m is None else _i32(m) for m in maps]
        parr = (ctypes.c_void_p * 3)(*[_p(m) for m in dmaps])
        offs_c, lens_c = (ctypes.c_int * 4)(*offs.tolist()), (ctypes.c_int * 3)(*lens.tolist())
        idx_d, slots_d = _i64(idx), _i32(slots)
        rows = torch.full((n + 8,), -7, dtype=torch.int32, device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        call('sbr_resolve_rows', _p(idx_d), k, _p(slots_d), n, 3, ctypes.cast(offs_c, ctypes.c_void_p), ctypes.cast(parr, ctypes.c_void_p),
             ctypes.cast(lens_c, ctypes.c_void_p), _p(rows), _p(err), stream())
        assert rows[:n].cpu().tolist() == want.tolist() and rows[n:].cpu().tolist() == [-7] * 8
        assert int(err) == int(miss) and (miss == with_missing or n == 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# sbr_scatter_add_rows: the D = 128 persistent-wave kernel, the one-element-per-thread power-of-two kernel, the grid-stride kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def _scatter_cases():
    cases = []
    for n in (4095, 4096, 4097, 4099):                                             # 4095: pow2 kernel at D = 128; from 4096 on the rows128 kernel
        cases.append((n, 128, 0, 0, 0, n % 2 == 1, 'random'))
    cases.append((4100, 128, 4, 8, 1, True, 'sorted'))                             # rows128 with strides, 4 bytes off, in_idx
    cases.append((4098, 128, 1, 3, 2, False, 'reversed'))
    cases.append((33_001, 128, 0, 0, 0, True, 'random'))                           # > 2,048 blocks x 16 rows: the persistent loop's second trip + clamped tail
    for D in (16, 32, 64, 128, 256):
        q = 256 // D
        for n in sorted({1, max(q - 1, 1), q, q + 1}):
            cases.append((n, D, 0, 0, 0, False, 'random'))
        cases.append((1501 + q, D, 3, 5, 1, True, 'sorted'))
    for D in (1, 3, 4, 12, 24, 68, 96, 100, 130, 260, 300):                        # grid-stride kernel
        cases.append((1, D, 0, 0, 0, False, 'random'))
        cases.append((1777, D, 2, 1, 2, True, 'reversed'))
    cases.append((349_600, 3, 0, 0, 0, False, 'random'))                           # 1,048,800 elements: second trip of the capped grid
    return cases


def _scatter_add_rows_run(n, D, xo, xw, off, use_ii, order, fill):
    """one sbr_scatter_add_rows call of a case of _scatter_cases into a table filled with ``fill`` -> (dW on the host, float64 sum of the
    sources per table row, sum of their magnitudes, sources per table row)"""
    n_table = 53
    rows = _orders(n, n_table, n * 31 + D, hot=11)[order]
    rng = np.random.default_rng(n + D)
    n_src = n + 5 if use_ii else n
    g = _rand(n_src, D, seed=n % 1000 + D)
    kind = rng.integers(0, 12, size=n_src)
    g[kind == 0] = 0.0
    g[kind == 1] = -0.0
    if D >= 2:
        g[torch.as_tensor(kind == 2), : (D + 1) // 2] = 0.0                      # zero first half
        g[torch.as_tensor(kind == 3), D // 2:] = 0.0                             # zero second half
    ii = rng.permutation(n_src)[:n] if use_ii else None
    dOut = _Buf(n_src, D, D + xo, off, data=g)
    dW = _Buf(n_table, D, D + xw, off, fill=fill)
    rows_d, ii_d = _i32(rows), (_i32(ii) if use_ii else None)
    call('sbr_scatter_add_rows', dOut.ptr, dOut.ld, _p(ii_d), _p(rows_d), dW.ptr, dW.ld, n, D, stream())
    got = dW.check_untouched(None, 'scatter_add_rows')
    src = g[torch.as_tensor(ii)] if use_ii else g
    rt = torch.as_tensor(rows, dtype=torch.int64)
    ref = torch.zeros(n_table, D, dtype=torch.float64).index_add_(0, rt, src.double())
    mag = torch.zeros(n_table, D, dtype=torch.float64).index_add_(0, rt, src.double().abs())
    m = torch.bincount(rt, minlength=n_table).double()[:, None]
    return got, ref, mag, m


@pytest.mark.parametrize('n,D,xo,xw,off,use_ii,order', _scatter_cases())
def test_scatter_add_rows(n, D, xo, xw, off, use_ii, order):
    """dW[rows[j], :] += dOut[ii(j), :] into a zeroed table: per element |err| <= m u sum|terms| with m the number of sources of that
    table row (m - 1 float atomic additions in any order; the first lands on +0 exactly). Rows that no source names stay +0 bit for bit.
    Gradient rows of zeros, of -0.0, with a zero first half and with a zero second half are mixed in (the D = 128 kernel skips all-zero
    rows by a ballot over both halves). One table row is named by 1,200 sources where n allows."""
    got, ref, mag, m = _scatter_add_rows_run(n, D, xo, xw, off, use_ii, order, 0.0)
    _assert_bound(got, ref, m * U32 * mag, f'scatter_add_rows n={n} D={D}')
    unnamed = m[:, 0] == 0
    assert bool((_bits(got[unnamed]) == 0).all()), 'a table row that no source names was written'


@pytest.mark.parametrize('n,D,xo,xw,off,use_ii,order', [(4097, 128, 0, 0, 0, True, 'random'),             # rows128 kernel
                                                        (4095, 128, 0, 0, 0, True, 'random'),             # pow2 kernel at D = 128
                                                        (1505, 64, 3, 5, 1, True, 'sorted'),              # pow2 kernel, strided
                                                        (1777, 100, 2, 1, 2, True, 'reversed'),           # grid-stride kernel
                                                        (5, 64, 0, 0, 0, False, 'random')])               # rows nobody names
def test_scatter_add_rows_adds_to_what_the_table_holds(n, D, xo, xw, off, use_ii, order):
    """The same cases, one per kernel, with dW prefilled with 0.5: the kernels ADD (a kernel that stored its sum would pass every test on
    a zeroed table). m atomic additions onto the existing value: |err| <= (m + 1) u (|dW| + sum|terms|), the bound of
    test_scatter_add_rows_sorted; rows that no source names keep 0.5 bit for bit."""
    got, ref, mag, m = _scatter_add_rows_run(n, D, xo, xw, off, use_ii, order, 0.5)
    _assert_bound(got, ref + 0.5, (m + 1) * U32 * (mag + 0.5), f'scatter_add_rows onto 0.5, n={n} D={D}')
    unnamed = m[:, 0] == 0
    assert bool(unnamed.any()) or n != 5
    _assert_bits(got[unnamed], torch.full_like(got[unnamed], 0.5), 'a table row that no source names was written')


# ---------------------------------------------------------------------------------------------------------------------------------
# sbr_bag_mean_fwd / _bwd
# ---------------------------------------------------------------------------------------------------------------------------------
def _bag_tags(n_ent, T, n_tags, pad, seed):
    rng = np.random.default_rng(seed)
    tags = rng.integers(0, n_tags, size=(n_ent, T))
    tags[tags == pad] = (pad + 1) % n_tags
    for e in range(n_ent):
        c = e % 5
        if c == 0:
            tags[e] = pad                                                          # all padding
        elif c == 1:
            tags[e, rng.integers(0, T)] = pad                                      # a pad in the middle of the list
        elif c == 2:
            tags[e, :] = tags[e, 0]                                                # one tag repeated T times
        elif c == 3:
            tags[e, T // 2:] = pad                                                 # padded tail
    return tags


@pytest.mark.parametrize('T', [1, 7, 40])
@pytest.mark.parametrize('n,D,xw,xo,off,use_oi', [(1, 1, 0, 0, 0, False), (3, 64, 0, 0, 0, True), (4, 65, 3, 0, 1, False), (5, 128, 0, 5, 2, True),
                                                  (259, 300, 4, 4, 0, True), (1000, 24, 1, 1, 1, False)])
def test_bag_mean_fwd_and_bwd(T, n, D, xw, xo, off, use_oi):
    """EmbeddingBag(mean, padding_idx): out[j] = mean over the non-pad tags of entity rows[j]; all-pad rows give zeros and no gradient.
    Forward: cnt - 1 additions, then the product with fl(1 / cnt) — two more roundings that the plain sum bound does not have — so
    |err| <= (cnt + 1) u sum|terms| / cnt (cnt <= T; with the issue's m = T this is T + 1 at most, the + 1 being the reciprocal).
    Backward: every source term is dOut * fl(1 / cnt) (two roundings), then m - 1 atomic additions for a tag of multiplicity m (counted
    over slots and repeats): |err| <= (m + 1) u sum|terms|. Four rows per block: n = 3, 4, 5."""
    n_ent, n_tags, pad = 23, 31, 4
    tags = _bag_tags(n_ent, T, n_tags, pad, T * 100 + D)
    rng = np.random.default_rng(n + T)
    rows = rng.integers(0, n_ent, size=n)
    if n >= 3:
        rows[0], rows[1], rows[2] = 0, 1, 2                                        # all-pad, pad in the middle, repeated tag
    W = _Buf(n_tags, D, D + xw, off, data=_rand(n_tags, D, seed=5))
    n_out = n + 2 if use_oi else n
    out = _Buf(n_out, D, D + xo, off)
    oi = rng.permutation(n_out)[:n] if use_oi else None
    tags_d, rows_d, oi_d = _i32(tags), _i32(rows), (_i32(oi) if use_oi else None)
    call('sbr_bag_mean_fwd', W.ptr, W.ld, _p(tags_d), T, pad, _p(rows_d), out.ptr, out.ld, _p(oi_d), n, D, stream())
    dst = torch.as_tensor(oi if use_oi else np.arange(n))
    got = out.check_untouched(dst, 'bag_mean_fwd')[dst]
    Wh = W.host().double()
    tg = torch.as_tensor(tags[rows])                                               # [n, T]
    live = (tg != pad)
    cnt = live.sum(1)
    terms = Wh[tg] * live[:, :, None]                                              # [n, T, D]
    den = cnt.clamp_min(1).double()[:, None]
    _assert_bound(got, terms.sum(1) / den, (cnt + 1).double()[:, None] * U32 * terms.abs().sum(1) / den, 'bag_mean_fwd')
    assert bool((_bits(got[cnt == 0]) == 0).all()), 'an all-padding row is not +0'
    # backward
    g = _rand(n_out, D, seed=6)
    dOut = _Buf(n_out, D, D + xo, off, data=g)
    dW = _Buf(n_tags, D, D + xw, off, fill=0.0)
    call('sbr_bag_mean_bwd', dOut.ptr, dOut.ld, _p(oi_d), _p(tags_d), T, pad, _p(rows_d), dW.ptr, dW.ld, n, D, stream())
    gotw = dW.check_untouched(None, 'bag_mean_bwd')
    contrib = (g[dst].double()[:, None, :] / den[:, :, None]) * live[:, :, None]   # [n, T, D]
    flat_t = tg.reshape(-1)
    ref = torch.zeros(n_tags, D, dtype=torch.float64).index_add_(0, flat_t, contrib.reshape(-1, D))
    mag = torch.zeros(n_tags, D, dtype=torch.float64).index_add_(0, flat_t, contrib.reshape(-1, D).abs())
    m = torch.zeros(n_tags, dtype=torch.float64).index_add_(0, flat_t, live.reshape(-1).double())[:, None]
    _assert_bound(gotw, ref, (m + 1) * U32 * mag, 'bag_mean_bwd')
    assert bool((_bits(gotw[m[:, 0] == 0]) == 0).all()) and bool((gotw[pad] == 0).all()), 'the padding tag or an unused tag received gradient'


# ---------------------------------------------------------------------------------------------------------------------------------
# sbr_l2norm_fwd / _bwd, ops.L2NormalizeFn
# ---------------------------------------------------------------------------------------------------------------------------------
def _l2_input(n, C, seed):
    """random rows plus the special ones: 0 zero row, 1 norm = eps / 2, 2 norm just above eps, 3 |x| ~ 1e-20, 4 |x| ~ 1e17"""
    eps = S().ops.NORM_EPS
    x = _rand(n, C, seed=seed)
    special = {}
    if n >= 5:
        x[0] = 0
        x[1] = 0; x[1, C // 2] = eps / 2
        x[2] = 0; x[2, 0] = -eps * 1.001
        x[3] = x[3] * 1e-20
        x[4] = x[4] * 1e17
        special = {'zero': 0, 'half_eps': 1, 'above_eps': 2, 'tiny': 3, 'huge': 4}
    return x, special


@pytest.mark.parametrize('C', [1, 24, 64, 65, 128, 300])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1030])
def test_l2norm_fwd_and_bwd(C, n):
    """F.normalize(x, dim=-1, eps) and its autograd gradient in float64 on the same fp32 input, through sbr_l2norm_fwd/_bwd and through
    ops.L2NormalizeFn (same bits). y: sum of C squares (relative error <= C u, all terms positive; the square root halves it), square
    root, reciprocal, product, and eps held in fp32: <= (C / 2 + 4) u, asserted as (C + 8) u |y|. dx: the same factor times
    inv (|dy| + |y| sum|y dy|), the magnitude of the terms of inv (dy - y (y . dy)) (the errors of inv, of the stored y and of the fp32
    dot product add up to (2.5 C + 11) u in the first-order worst case, when every rounding of the C squares and of the C products of
    the dot falls the same way; the asserted (C + 8) u is the tighter figure the row-wise kernels are held to). The clamped rows (norm <= eps: zero row, eps / 2,
    |x| ~ 1e-20) are compared like every other row: there dx = dy / eps. No row is left out. The 1e-20 row squares into fp32 denormals,
    which only decides that it is clamped; the 1e17 row keeps C x^2 below the fp32 maximum."""
    ops = S().ops
    eps = ops.NORM_EPS
    x, special = _l2_input(n, C, 40 + C)
    dy = _rand(n, C, seed=41 + C)
    xr = x.double().requires_grad_(True)
    yr = torch.nn.functional.normalize(xr, p=2, dim=-1, eps=eps)
    (yr * dy.double()).sum().backward()
    yr = yr.detach()
    X, Y, INV = _Buf(n, C, data=x), _Buf(n, C), _Buf(1, n)
    call('sbr_l2norm_fwd', X.ptr, Y.ptr, INV.ptr, n, C, eps, stream())
    y = Y.check_untouched(None, 'l2norm_fwd y')
    inv = INV.check_untouched(None, 'l2norm_fwd inv')[0]
    fac = (C + 8) * U32
    _assert_bound(y, yr, fac * yr.abs(), 'l2norm y')
    inv_ref = 1.0 / x.double().norm(dim=1).clamp_min(eps)
    _assert_bound(inv, inv_ref, fac * inv_ref, 'l2norm inv')
    DY, DX = _Buf(n, C, data=dy), _Buf(n, C)
    call('sbr_l2norm_bwd', DY.ptr, Y.ptr, INV.ptr, DX.ptr, n, C, eps, stream())
    dx = DX.check_untouched(None, 'l2norm_bwd')
    bound = fac * inv_ref[:, None] * (dy.double().abs() + yr.abs() * (yr * dy.double()).abs().sum(1, keepdim=True))
    _assert_bound(dx, xr.grad, bound, 'l2norm dx')
    if special:
        clamped = [special['zero'], special['half_eps'], special['tiny']]
        assert bool((x[clamped].double().norm(dim=1) < eps).all()) and float(x[special['above_eps']].double().norm()) > eps
        _assert_bound(dx[clamped], dy[clamped].double() / eps, 3 * U32 * dy[clamped].double().abs() / eps, 'l2norm dx of the clamped rows')
        assert bool((dx[special['above_eps']][1:] != 0).any()) or C == 1
    # the autograd wrapper runs the same two kernels
    xd = x.to(DEV).requires_grad_(True)
    yw = ops.L2NormalizeFn.apply(xd)
    (yw * dy.to(DEV)).sum().backward()
    _assert_bits(yw.detach().cpu(), y, 'L2NormalizeFn y')
    _assert_bits(xd.grad.cpu(), dx, 'L2NormalizeFn dx')


# ---------------------------------------------------------------------------------------------------------------------------------
# sbr_aggregate_fwd / _bwd, ops.AggregateFn
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S_,k,D', [(1, 1, 1), (13, 2, 9), (255, 3, 1), (257, 8, 3), (5, 255, 68), (64, 3, 128), (8200, 2, 128), (3501, 3, 300)])
def test_aggregate_fwd_and_bwd(S_, k, D):
    """E [S, k, D] -> mean / max over dim 1. max: the value bit for bit, the gradient goes to the FIRST maximal index (exact ties between
    modalities are planted in every third slot). mean: k - 1 additions and one division: |err| <= k u sum|terms| / k; its gradient is
    dOut / k (one rounding: 1 u). (8200, 2, 128) and (3501, 3, 300) are above the 1,048,576-element grid cap in both directions."""
    ops = S().ops
    e = _rand(S_, k, D, seed=S_ + k)
    if k >= 2:
        e[::3, k - 1] = e[::3, 0]                                                  # first and last modality tie exactly ...
        e[::6, 0] = e[::6].max(1).values                                           # ... and in every sixth slot the tie IS the maximum
    g = _rand(S_, D, seed=7)
    E, G = _Buf(S_, k * D, data=e.reshape(S_, k * D)), _Buf(S_, D, data=g)
    ed = e.double()
    for mode in (0, 1):
        out, dE = _Buf(S_, D), _Buf(S_, k * D)
        arg = torch.full((S_ * D + 64,), 251, dtype=torch.uint8, device=DEV)
        call('sbr_aggregate_fwd', E.ptr, out.ptr, _p(arg) if mode == 1 else None, S_, k, D, mode, stream())
        o = out.check_untouched(None, 'aggregate_fwd')
        call('sbr_aggregate_bwd', G.ptr, _p(arg) if mode == 1 else None, dE.ptr, S_, k, D, mode, stream())
        de = dE.check_untouched(None, 'aggregate_bwd').reshape(S_, k, D)
        if mode == 0:
            _assert_bound(o, ed.mean(1), k * U32 * ed.abs().sum(1) / k, 'aggregate mean')
            _assert_bound(de, (g.double() / k)[:, None, :].expand(S_, k, D), U32 * (g.double().abs() / k)[:, None, :].expand(S_, k, D), 'aggregate mean grad')
            assert bool((arg == 251).all())
        else:
            mx = e.max(1).values
            _assert_bits(o, mx, 'aggregate max')
            first = torch.where(e == mx[:, None, :], torch.arange(k)[None, :, None], k).min(1).values          # first maximal index
            assert torch.equal(arg[:S_ * D].cpu().long().view(S_, D), first) and bool((arg[S_ * D:] == 251).all())
            ref = torch.zeros(S_, k, D).scatter_(1, first[:, None, :], g[:, None, :])
            _assert_bits(de, ref, 'aggregate max grad')
        if S_ * k * D <= 300_000:                                                  # the autograd wrapper: the same kernels
            edv = e.to(DEV).requires_grad_(True)
            ow = ops.AggregateFn.apply(edv, mode)
            (ow * g.to(DEV)).sum().backward()
            _assert_bits(ow.detach().cpu(), o, 'AggregateFn')
            _assert_bits(edv.grad.cpu(), de, 'AggregateFn grad')


# ---------------------------------------------------------------------------------------------------------------------------------
# sbr_dropout / sbr_dropout_dev, ops.DropoutFn
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', [0.0, 0.2, 0.5, 0.999])
def test_dropout_properties(p):
    """Counter-based dropout, y = keep(seed, e) ? x / (1 - p) : 0. The kernel multiplies by fl(1 / fl(1 - p)); for the p of this test the
    fp32 scale is within 0.5 u of the exact 1 / (1 - p32) (1 - p is exact for p >= 0.5 and for 0; asserted below on the CPU), so a kept
    element is within 1 ulp of x / (1 - p32): half an ulp of the product's rounding plus the scale's error. p = 0 is the identity bit for
    bit. The mask is a function of (seed, element index) alone: shared by forward and backward, equal between sbr_dropout(seed s) and
    sbr_dropout_dev(seed_dev = a, offset = s - a), and independent of the launch geometry (1,000 vs 3,000,000 elements; the latter is
    above the 1,048,576-element grid cap). Keep rate within 4 binomial standard deviations of 1 - p."""
    p32 = float(np.float32(p))
    scale32 = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    assert abs(scale32 * (1.0 - p32) - 1.0) <= 0.5 * U32, 'the fp32 scale of this p is not within one rounding of 1 / (1 - p)'
    n_big, n_small, seed = 3_000_000, 1000, 123_456_789
    x = _rand(n_big, seed=8) + 3.0 * torch.sign(_rand(n_big, seed=9))              # no zeros: a dropped element is recognisable
    X, Yb, Ys, Yd, G, DXb = _Buf(1, n_big, data=x[None]), _Buf(1, n_big), _Buf(1, n_small, off=1), _Buf(1, n_big, off=2), None, None
    call('sbr_dropout', X.ptr, Yb.ptr, n_big, p, seed, stream())
    call('sbr_dropout', X.ptr, Ys.ptr, n_small, p, seed, stream())
    seed_dev = torch.tensor([seed - 1000], dtype=torch.int64, device=DEV)
    call('sbr_dropout_dev', X.ptr, Yd.ptr, n_big, p, _p(seed_dev), 1000, stream())
    yb, ys, yd = Yb.check_untouched(None, 'dropout')[0], Ys.check_untouched(None, 'dropout small')[0], Yd.check_untouched(None, 'dropout_dev')[0]
    _assert_bits(yd, yb, 'sbr_dropout_dev(a, s - a) vs sbr_dropout(s)')
    _assert_bits(ys, yb[:n_small], 'the mask depends on the launch geometry')
    kept = yb != 0
    if p == 0.0:
        _assert_bits(yb, x, 'p = 0 is not the identity')
    ref = x.double() / (1.0 - p32)
    err = (yb.double() - ref).abs()
    assert bool((err[kept] <= _ulp(ref)[kept]).all()), f'a kept element is off by {float((err / _ulp(ref))[kept].max())} ulp'
    assert bool((_bits(yb[~kept]) == 0).all())
    rate, sd = float(kept.double().mean()), math.sqrt(p32 * (1 - p32) / n_big)
    assert abs(rate - (1 - p32)) <= 4 * sd, f'keep rate {rate} vs {1 - p32} (sd {sd})'
    # backward of the same seed: the same mask on another tensor; another seed: another mask
    g = _rand(n_small, seed=10) + 3.0
    Gb, DX = _Buf(1, n_small, data=g[None]), _Buf(1, n_small)
    call('sbr_dropout', Gb.ptr, DX.ptr, n_small, p, seed, stream())
    assert torch.equal(DX.check_untouched(None, 'dropout bwd')[0] != 0, kept[:n_small])
    if 0 < p < 0.9:
        call('sbr_dropout', Gb.ptr, DX.ptr, n_small, p, seed + 1, stream())
        assert not torch.equal(DX.host()[0] != 0, kept[:n_small])
    xd = x[:n_small].to(DEV).requires_grad_(True)
    yw = S().ops.DropoutFn.apply(xd, p, seed)
    _assert_bits(yw.detach().cpu(), yb[:n_small], 'DropoutFn')
    yw.sum().backward()
    assert torch.equal(xd.grad.cpu() != 0, kept[:n_small])


# ---------------------------------------------------------------------------------------------------------------------------------
# sbr_score_dot_fwd / _bwd, ops.ScoreDotFn
# ---------------------------------------------------------------------------------------------------------------------------------
def _score_dot_cases():
    cases = []
    for q, D in enumerate(DS):
        N = (1, 2, 11, 16)[q % 4]
        cases.append((5, N, D, 0, 0))
        if D % 4 == 0 and D <= 256:
            cases.append((3, (2, 11, 16, 1)[q % 4], D, 1, 0))                      # U 4 bytes off -> one wave per slot
            cases.append((7, 11, D, 0, 2))                                         # I 8 bytes off -> one wave per slot
    cases += [(1, 1, 64, 0, 0), (1, 1, 128, 0, 0), (1, 1, 256, 0, 0), (1, 1, 300, 0, 0), (1031, 11, 64, 0, 0), (513, 3, 128, 0, 0), (300, 11, 256, 0, 0),
              (257, 1, 12, 0, 0), (129, 2, 68, 0, 0)]
    return cases


@pytest.mark.parametrize('B,N,D,off_u,off_i', _score_dot_cases())
def test_score_dot_fwd_and_bwd(B, N, D, off_u, off_i):
    """einsum('be,bce->bc'): |err| <= D u sum_d|u_d i_d| (D products and D - 1 additions, fused or not, in any order). float4 kernel with
    16 / 32 / 64 lanes per slot for D % 4 == 0, D <= 256 and 16-byte aligned operands (D = 12: 3 of 16 lanes live, D = 68: 17 of 32),
    else one wave per slot; B N is mostly not a multiple of the slots per wave. Backward (64 / 128 / 256 threads by D):
    dU = sum_n g_n i_n within N u sum|g_n i_nd|, dI = g u within one rounding (1 u relative, <= 1 ulp); null dU / null dI leave the other
    unchanged in bits."""
    u, it, g = _rand(B, D, seed=B + D), _rand(B, N, D, seed=N + D), _rand(B, N, seed=11)
    Ub, Ib, out = _Buf(B, D, off=off_u, data=u), _Buf(B, N * D, off=off_i, data=it.reshape(B, N * D)), _Buf(B, N, off=1)
    call('sbr_score_dot_fwd', Ub.ptr, Ib.ptr, out.ptr, B, N, D, stream())
    o = out.check_untouched(None, 'score_dot_fwd')
    ud, idd, gd = u.double(), it.double(), g.double()
    _assert_bound(o, torch.einsum('be,bce->bc', ud, idd), D * U32 * torch.einsum('be,bce->bc', ud.abs(), idd.abs()), 'score_dot_fwd')
    Gb = _Buf(B, N, data=g)
    res = {}
    for which in ('both', 'dU', 'dI'):
        dU, dI = (_Buf(B, D, off=off_u) if which != 'dI' else None), (_Buf(B, N * D, off=off_i) if which != 'dU' else None)
        call('sbr_score_dot_bwd', Gb.ptr, Ub.ptr, Ib.ptr, dU.ptr if dU else None, dI.ptr if dI else None, B, N, D, stream())
        res[which] = (dU.check_untouched(None, 'dU') if dU else None, dI.check_untouched(None, 'dI') if dI else None)
    du, di = res['both']
    _assert_bound(du, torch.einsum('bn,bnd->bd', gd, idd), N * U32 * torch.einsum('bn,bnd->bd', gd.abs(), idd.abs()), 'score_dot dU')
    di_ref = gd[:, :, None] * ud[:, None, :]
    _assert_bound(di.reshape(B, N, D), di_ref, U32 * di_ref.abs(), 'score_dot dI')
    _assert_bits(res['dU'][0], du, 'dU with a null dI')
    _assert_bits(res['dI'][1], di, 'dI with a null dU')
    if off_u == 0 and off_i == 0:
        ops = S().ops
        uw, iw = u.to(DEV).requires_grad_(True), it.to(DEV).requires_grad_(True)
        ow = ops.ScoreDotFn.apply(uw, iw)
        _assert_bits(ow.detach().cpu(), o, 'ScoreDotFn')
        (ow * g.to(DEV)).sum().backward()
        _assert_bits(uw.grad.cpu(), du, 'ScoreDotFn dU')
        _assert_bits(iw.grad.cpu().reshape(B, N * D), di, 'ScoreDotFn dI')
        u2 = u.to(DEV).requires_grad_(True)                                        # only dU needed: the wrapper passes a null dI
        (ops.ScoreDotFn.apply(u2, it.to(DEV)) * g.to(DEV)).sum().backward()
        _assert_bits(u2.grad.cpu(), du, 'ScoreDotFn dU alone')


# ---------------------------------------------------------------------------------------------------------------------------------
# bias scorers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,N', [(1, 1), (85, 3), (86, 3), (255, 1), (257, 11), (1, 300)])
def test_bias_score_fwd_add_and_bwd(B, N):
    """out[b, n] = base + user_bias[u[b] or b] + item_bias[i[b, n] or n] + global_bias, every term and both index lists optional
    (sbr_bias_score_add_fwd: all 64 combinations of null operands; sbr_bias_score_fwd: the all-given form; ops.BiasScoreFn). At most four
    terms, three additions: |err| <= 3 u sum|terms|. Backward (all 32 combinations): the scatter-add bound, m sources per table entry
    (m u sum|terms|; B N for the global bias, whose block sums are m - 1 additions in another order)."""
    nu, ni = max(B, 40), max(N, 50)
    ub, ib, gb, base = _rand(nu, seed=12), _rand(ni, seed=13), _rand(1, seed=14) , _rand(B, N, seed=15)
    rng = np.random.default_rng(B * N)
    u, i = rng.integers(0, nu, size=B), rng.integers(0, ni, size=(B, N))
    if B > 4:
        i[:, 0] = 5                                                                # a hot item
    ub_d, ib_d, gb_d, base_d, u_d, i_d = _dev(ub), _dev(ib), _dev(gb), _dev(base), _i64(u), _i64(i)
    g = _rand(B, N, seed=16)
    g_d = _dev(g)
    bb, nn = torch.arange(B)[:, None].expand(B, N), torch.arange(N)[None, :].expand(B, N)
    for mask in range(64):
        h_ub, h_ib, h_gb, h_base, h_u, h_i = [(mask >> q) & 1 for q in range(6)]
        ui = torch.as_tensor(u)[:, None].expand(B, N) if h_u else bb
        ii = torch.as_tensor(i) if h_i else nn
        terms = [base.double() if h_base else None, ub.double()[ui] if h_ub else None, ib.double()[ii] if h_ib else None,
                 gb.double().expand(B, N) if h_gb else None]
        terms = [t for t in terms if t is not None]
        ref = sum(terms) if terms else torch.zeros(B, N, dtype=torch.float64)
        mag = sum(t.abs() for t in terms) if terms else torch.zeros(B, N, dtype=torch.float64)
        out = _Buf(1, B * N, off=mask % 3)
        call('sbr_bias_score_add_fwd', _p(ub_d) if h_ub else None, _p(ib_d) if h_ib else None, _p(gb_d) if h_gb else None,
             _p(u_d) if h_u else None, _p(i_d) if h_i else None, _p(base_d) if h_base else None, out.ptr, B, N, stream())
        o = out.check_untouched(None, f'bias_score_add_fwd {mask:06b}')[0].view(B, N)
        _assert_bound(o, ref, 3 * U32 * mag, f'bias_score_add_fwd {mask:06b}')
        if mask == 0b110111:                                                       # no base, everything else: sbr_bias_score_fwd is the same sum
            out2 = _Buf(1, B * N)
            call('sbr_bias_score_fwd', _p(ub_d), _p(ib_d), _p(gb_d), _p(u_d), _p(i_d), out2.ptr, B, N, stream())
            _assert_bits(out2.check_untouched(None, 'bias_score_fwd')[0].view(B, N), o, 'sbr_bias_score_fwd vs the add form')
    gdb = g.double()
    for mask in range(32):
        h_ub, h_ib, h_gb, h_u, h_i = [(mask >> q) & 1 for q in range(5)]
        d_ub, d_ib, d_gb = (_Buf(1, nu, fill=0.0) if h_ub else None), (_Buf(1, ni, fill=0.0) if h_ib else None), (_Buf(1, 1, fill=0.0) if h_gb else None)
        call('sbr_bias_score_bwd', _p(g_d), _p(u_d) if h_u else None, _p(i_d) if h_i else None, d_ub.ptr if d_ub else None,
             d_ib.ptr if d_ib else None, d_gb.ptr if d_gb else None, B, N, stream())
        ui = (torch.as_tensor(u)[:, None].expand(B, N) if h_u else bb).reshape(-1)
        ii = (torch.as_tensor(i) if h_i else nn).reshape(-1)
        for buf, ix, size in ((d_ub, ui, nu), (d_ib, ii, ni)):
            if buf is None:
                continue
            ref = torch.zeros(size, dtype=torch.float64).index_add_(0, ix, gdb.reshape(-1))
            mag = torch.zeros(size, dtype=torch.float64).index_add_(0, ix, gdb.reshape(-1).abs())
            m = torch.bincount(ix, minlength=size).double()
            _assert_bound(buf.check_untouched(None, 'bias bwd')[0], ref, m * U32 * mag, f'bias_score_bwd {mask:05b}')
        if d_gb is not None:
            _assert_bound(d_gb.check_untouched(None, 'bias bwd global')[0], gdb.sum().reshape(1), (B * N * U32 * gdb.abs().sum()).reshape(1), 'bias_score_bwd global')
    # the autograd wrapper, everything given
    ops = S().ops
    ts = [t.clone().requires_grad_(True) for t in (base_d, ub_d, ib_d, gb_d)]
    ow = ops.BiasScoreFn.apply(ts[0], ts[1], ts[2], ts[3], u_d, i_d, B, N)
    ref = base.double() + ub.double()[torch.as_tensor(u)][:, None] + ib.double()[torch.as_tensor(i)] + gb.double()
    _assert_bound(ow.detach().cpu(), ref, 3 * U32 * (base.double().abs() + ub.double().abs()[torch.as_tensor(u)][:, None] + ib.double().abs()[torch.as_tensor(i)] + gb.double().abs()), 'BiasScoreFn')
    (ow * g_d).sum().backward()
    _assert_bits(ts[0].grad.cpu(), g, 'BiasScoreFn d base')
    ix = torch.as_tensor(i).reshape(-1)
    _assert_bound(ts[2].grad.cpu(), torch.zeros(ni, dtype=torch.float64).index_add_(0, ix, gdb.reshape(-1)),
                  torch.bincount(ix, minlength=ni).double() * U32 * torch.zeros(ni, dtype=torch.float64).index_add_(0, ix, gdb.reshape(-1).abs()), 'BiasScoreFn d item_bias')
    _assert_bound(ts[3].grad.cpu(), gdb.sum().reshape(1), (B * N * U32 * gdb.abs().sum()).reshape(1), 'BiasScoreFn d global_bias')


# ---------------------------------------------------------------------------------------------------------------------------------
# sbr_csr_rows_to_dense
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dim,xo,with_data', [(1, 0, True), (255, 0, False), (256, 3, True), (257, 1, False), (5000, 8, True)])
def test_csr_rows_to_dense(dim, xo, with_data):
    """out[j, :] = row ent[j] of the CSR matrix as a dense vector (``matrix[ent].toarray()``), all zeros for ent[j] = -1 and for empty
    rows; data null: ones. Bit-exact. One row holds min(dim, 3,500) entries, ldo > dim leaves the padding columns alone."""
    import scipy.sparse as sp
    rng = np.random.default_rng(dim)
    n_rows = 12
    lens = [0, min(dim, 3500), 1, 0, min(dim, 7), min(dim, 64), min(dim, 300), 0, 1, min(dim, 2), min(dim, 256), min(dim, 257)]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(dim, size=l, replace=False)) for l in lens]).astype(np.int32)
    data = rng.standard_normal(indices.size).astype(np.float32)
    dense = torch.from_numpy(sp.csr_matrix((data if with_data else np.ones_like(data), indices, indptr), shape=(n_rows, dim)).toarray())
    ent = np.array([1, -1, 0, 1, 5, 11, -1, 3, 2, 10, 6, 4, 9, 8, 7, 1])
    n = len(ent)
    ref = torch.where(torch.as_tensor(ent >= 0)[:, None], dense[torch.as_tensor(np.maximum(ent, 0))], torch.zeros(n, dim))
    ip, ix, dv, en = _i64(indptr), _i32(indices), (torch.from_numpy(data).to(DEV) if with_data else None), _i64(ent)
    out = _Buf(n, dim, dim + xo, off=1)
    call('sbr_csr_rows_to_dense', _p(ip), _p(ix), _p(dv), _p(en), n, dim, out.ptr, out.ld, stream())
    _assert_bits(out.check_untouched(None, 'csr_rows_to_dense'), ref, 'csr_rows_to_dense')
    with pytest.raises(_L().SibrarHipError):
        call('sbr_csr_rows_to_dense', _p(ip), _p(ix), _p(dv), _p(en), n, dim, out.ptr, dim - 1, stream())


# ---------------------------------------------------------------------------------------------------------------------------------
# the scalar branches of sbr_act_grad_gather, sbr_colsum, sbr_csr_project_fwd / _bwd (the float4 / workgroup branches have their tests
# in test_hip_kernels.py)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,C,xl,xz,off,use_ii', [(7, 30, 0, 0, 0, True), (64, 64, 1, 0, 0, False), (65, 64, 0, 2, 0, True), (33, 128, 0, 0, 1, False),
                                                  (5, 12, 0, 0, 2, True), (8200, 129, 0, 0, 0, True), (300, 64, 4, 8, 0, True)])
@pytest.mark.parametrize('act', [0, 1, 2, 3])
def test_act_grad_gather_scalar_branch(n, C, xl, xz, off, use_ii, act):
    """dZ[j] = dY[ii(j)] * act'(Y[ii(j)]) with act' from the activation OUTPUT (1, y > 0, 1 - y^2, y (1 - y)): C % 4 != 0, ld or ldz not a
    multiple of 4, or a base pointer off 16 bytes runs the scalar kernel ((8200, 129): above its grid cap); the last case is the float4
    kernel with strided views. At most three roundings: |err| <= 3 u |dy| (1 + y^2)."""
    n_src = n + 4
    dy = _rand(n_src, C, seed=17)
    y = torch.tanh(_rand(n_src, C, seed=18)) if act != 3 else torch.sigmoid(_rand(n_src, C, seed=18))
    if act == 1:
        y = torch.relu(y)
    DY, Y = _Buf(n_src, C, C + xl, off, data=dy), _Buf(n_src, C, C + xl, off, data=y)
    DZ = _Buf(n, C, C + xz, off)
    ii = np.random.default_rng(n).integers(0, n_src, size=n)
    ii_d = _i32(ii) if use_ii else None
    call('sbr_act_grad_gather', DY.ptr, Y.ptr, DY.ld, _p(ii_d), DZ.ptr, DZ.ld, n, C, act, stream())
    sel = torch.as_tensor(ii) if use_ii else torch.arange(n)
    d, yy = dy[sel].double(), y[sel].double()
    ref = d * {0: torch.ones_like(yy), 1: (yy > 0).double(), 2: 1 - yy * yy, 3: yy * (1 - yy)}[act]
    _assert_bound(DZ.check_untouched(None, 'act_grad_gather'), ref, 3 * U32 * d.abs() * (1 + yy * yy), 'act_grad_gather')


@pytest.mark.parametrize('n,C,xl,off', [(1, 1, 0, 0), (63, 30, 0, 0), (64, 64, 1, 0), (65, 64, 0, 1), (40_000, 130, 2, 0), (257, 1028, 0, 0), (100, 64, 4, 0)])
def test_colsum_generic_branch(n, C, xl, off):
    """out[c] = sum_j X[j, c]. C % 4 != 0, C > 1024, ld % 4 != 0 or a misaligned base take the generic kernel (40,000 rows: above its
    512 x 4 row groups), which accumulates in float64 and rounds to fp32 once: |err| <= u |sum| + n 2^-53 sum|terms|. The last case is the
    float4 kernel on a strided view: its threads add their rows in fp32 before the float64 combination (colred.h, sbr_col_reduce), an
    fp32 sum of at most n terms: + n u sum|terms|. The workspace (17 C doubles, zeroed once) is left zeroed by the call."""
    x = _rand(n, C, seed=19)
    X, out = _Buf(n, C, C + xl, off, data=x), _Buf(1, C, off=1)
    ws = torch.zeros(17 * C, dtype=torch.float64, device=DEV)
    for _ in range(2):                                                             # the second call runs on the workspace the first one left
        out.flat.fill_(NAN)
        call('sbr_colsum', X.ptr, X.ld, n, C, out.ptr, _p(ws), stream())
        ref = x.double().sum(0)
        f4 = C % 4 == 0 and C <= 1024 and X.ld % 4 == 0 and off == 0
        _assert_bound(out.check_untouched(None, 'colsum')[0], ref, U32 * ref.abs() + n * (U32 if f4 else 2.0 ** -53) * x.double().abs().sum(0), 'colsum')
        assert bool((ws == 0).all()), 'the workspace is not left zeroed'


@pytest.mark.parametrize('C,xw,off,with_vals', [(64, 0, 1, True), (64, 2, 0, False), (516, 0, 2, True), (7, 0, 0, True),
                                                (64, 4, 0, True), (128, 0, 0, False), (200, 0, 0, True), (512, 8, 0, False)])
def test_csr_project_branches(C, xw, off, with_vals):
    """sbr_csr_project_fwd with a misaligned weight base or ldw % 4 != 0 at C % 4 == 0 (wave-per-row kernel; test_hip_kernels.py reaches
    it through C = 30 only) and sbr_csr_project_bwd at C > 512 (the generic kernel: more than eight 64-column chunks). A row of q nnz:
    q products, q additions (bias): |err| <= (q + 1) u sum|terms|; dWt[col] gets m sources: (m + 1) u sum|terms| (the + 1: the product
    val * g of every source). The four aligned cases run the workgroup-per-row kernels of both directions (1, 2, 4 and 8 column chunks
    per lane) on strided views, and the backward pass in its gather form (sbr_csr_project_bwd_gather: slot gradients added per entity,
    then every feature column sums its entities' rows over the transposed matrix and adds to dWt; a source passes k_e - 1 + 1 + E_c - 1
    + 1 <= m + 1 roundings: (m + 2) u sum|terms|)."""
    rng = np.random.default_rng(C)
    n_rows, n_cols = 9, 40
    lens = [0, 1, 40, 7, 13, 0, 2, 33, 5]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(n_cols, size=l, replace=False)) for l in lens]).astype(np.int32)
    vals = rng.standard_normal(indices.size).astype(np.float32)
    dense = torch.zeros(n_rows, n_cols, dtype=torch.float64)
    for r in range(n_rows):
        dense[r, indices[indptr[r]:indptr[r + 1]].astype(np.int64)] = torch.from_numpy(vals[indptr[r]:indptr[r + 1]]).double() if with_vals else 1.0
    wt, b = _rand(n_cols, C, seed=20), _rand(C, seed=21)
    rows = np.array([2, 0, 1, 2, 8, 7, 3, 4, 5, 6, 2])
    n = len(rows)
    Wt, out = _Buf(n_cols, C, C + xw, off, data=wt), _Buf(n + 2, C, C + 1, 0)
    oi = rng.permutation(n + 2)[:n]
    ip, ix, dv, rows_d, oi_d, b_d = _i64(indptr), _i32(indices), (torch.from_numpy(vals).to(DEV) if with_vals else None), _i32(rows), _i32(oi), _dev(b)
    call('sbr_csr_project_fwd', _p(ip), _p(ix), _p(dv), Wt.ptr, Wt.ld, _p(b_d), _p(rows_d), out.ptr, out.ld, _p(oi_d), n, C, 0, stream())
    got = out.check_untouched(torch.as_tensor(oi), 'csr_project_fwd')[torch.as_tensor(oi)]
    d = dense[torch.as_tensor(rows)]
    q = (d != 0).sum(1, keepdim=True).double()
    _assert_bound(got, d @ wt.double() + b.double(), (q + 1) * U32 * (d.abs() @ wt.double().abs() + b.double().abs()), 'csr_project_fwd')
    dz = _rand(n, C, seed=22)
    dZ, dWt = _Buf(n, C, C + 3, off, data=dz), _Buf(n_cols, C, C + xw, off, fill=0.0)
    call('sbr_csr_project_bwd', _p(ip), _p(ix), _p(dv), dZ.ptr, dZ.ld, _p(rows_d), dWt.ptr, dWt.ld, n, C, stream())
    m = (d != 0).sum(0).double()[:, None]
    _assert_bound(dWt.check_untouched(None, 'csr_project_bwd'), d.t() @ dz.double(), (m + 1) * U32 * (d.abs().t() @ dz.double().abs()), 'csr_project_bwd')
    if C % 4 == 0 and xw % 4 == 0 and off == 0:
        import scipy.sparse as sp
        mt = sp.csr_matrix((vals if with_vals else np.ones_like(vals), indices, indptr), shape=(n_rows, n_cols)).T.tocsr()
        mt.sort_indices()
        tp, tx, tv = _i64(mt.indptr), _i32(mt.indices), (torch.from_numpy(mt.data.astype(np.float32)).to(DEV) if with_vals else None)
        dZe, dWt2 = _Buf(n_rows, C), _Buf(n_cols, C, C + xw, 0, fill=0.25)
        call('sbr_csr_project_bwd_gather', _p(tp), _p(tx), _p(tv), dZ.ptr, dZ.ld, None, _p(rows_d), n, dZe.ptr, C, n_rows, dWt2.ptr, dWt2.ld,
             n_cols, C, stream())
        dZe.check_untouched(None, 'csr_project_bwd_gather workspace')
        _assert_bound(dWt2.check_untouched(None, 'csr_project_bwd_gather'), d.t() @ dz.double() + 0.25,
                      (m + 2) * U32 * (d.abs().t() @ dz.double().abs() + 0.25), 'csr_project_bwd_gather')


# ---------------------------------------------------------------------------------------------------------------------------------
# the casts of the fused scorers
# ---------------------------------------------------------------------------------------------------------------------------------
def _f32_sweep():
    """all 256 fp32 exponents x mantissa patterns, both signs; +-0, +-inf, NaN, the fp16 overflow (65504 / 65520) and denormal
    (2^-14, 2^-24, 2^-25) edges with their neighbours"""
    man = np.array([0, 1, 2, 0x0FFF, 0x1000, 0x1001, 0x1FFF, 0x2000, 0x2001, 0x3000, 0x7FFF, 0x8000, 0x8001, 0x17FFF, 0x18000, 0x18001, 0x3FFFFF, 0x400000,
                    0x400001, 0x555555, 0x2AAAAA, 0x7F0000, 0x7FEFFF, 0x7FF000, 0x7FFFFE, 0x7FFFFF, 0x123456, 0x654321], dtype=np.uint32)
    exp = np.arange(256, dtype=np.uint32)
    bits = ((exp[:, None] << 23) | man[None, :]).reshape(-1)
    edges = np.array([65504.0, 65519.99, 65520.0, 65520.01, 65536.0, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -11), 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20),
                      2.0 ** -26, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 0.0, 1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11], dtype=np.float32).view(np.uint32)
    bits = np.concatenate([bits, edges, np.random.default_rng(5).integers(0, 2 ** 32, size=200_000, dtype=np.uint64).astype(np.uint32)])
    bits = np.concatenate([bits, bits ^ np.uint32(0x80000000)])
    return torch.from_numpy(bits.view(np.int32).copy()).view(torch.float32)


def test_cast_f32_to_f16_is_round_to_nearest_even():
    """sbr_cast_f32_to_f16 == x.half() on the CPU bit for bit (NaN-ness for NaN) over the sweep, and over 2,200,000 elements (above the
    8,192-block grid cap)."""
    x = _f32_sweep()
    x = torch.cat([x, _rand(2_200_000 - x.numel() % 7, seed=23) * 300])
    n = x.numel()
    assert n > 8192 * 256
    X = _Buf(1, n, data=x[None])
    Y = _Buf(1, n, off=1, dtype=torch.float16)
    call('sbr_cast_f32_to_f16', X.ptr, Y.ptr, n, stream())
    got, ref = Y.check_untouched(None, 'cast_f16')[0], x.half()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(got[~nan].view(torch.int16), ref[~nan].view(torch.int16)), 'sbr_cast_f32_to_f16 differs from round-to-nearest-even'
    assert torch.equal(S().ops.cast_f16(x[:1000].to(DEV)).cpu().view(torch.int16)[~nan[:1000]], ref[:1000].view(torch.int16)[~nan[:1000]])


SPLIT_LO, SPLIT_HI = 2.0 ** -100, 3.38e38          # ops.split_bf16x3 is exact for x = 0 and SPLIT_LO <= |x| <= SPLIT_HI


def test_split_f32_to_bf16x3_planes_and_exactness_range():
    """sbr_split_f32_to_bf16x3: p0 = bf16(x), p1 = bf16(x - p0), p2 = bf16((x - p0) - p1), round to nearest even — the planes are bit
    identical to that chain in torch on the CPU over the sweep (finite x; inf / NaN give non-finite planes and are compared by NaN-ness),
    and p0 + p1 + p2 == x in float64 for x = 0 and SPLIT_LO <= |x| <= SPLIT_HI: 8 + 8 + 8 significand bits cover the 24 of fp32 as long
    as the third plane, up to 2^-16 |x| (two roundings of half a bf16 ulp each), neither underflows bf16 (|x| >= 2^-100 keeps it above
    2^-126 with its 8 bits) nor the first plane rounds to inf (|x| > 3.3961e38 does). 2,200,000 elements: above the 8,192-block grid cap."""
    x = _f32_sweep()
    x = torch.cat([x, _rand(2_200_000 - x.numel(), seed=24)])
    n = x.numel()
    assert n > 8192 * 256
    p0 = x.bfloat16()
    r1 = x - p0.float()
    p1 = r1.bfloat16()
    p2 = (r1 - p1.float()).bfloat16()
    ref = torch.stack([p0, p1, p2])
    X = _Buf(1, n, data=x[None])
    Y = _Buf(3, n, dtype=torch.bfloat16)
    call('sbr_split_f32_to_bf16x3', X.ptr, Y.ptr, n, stream())
    got = Y.check_untouched(None, 'split_bf16x3')
    nan = torch.isnan(ref.float())
    assert torch.equal(torch.isnan(got.float()), nan)
    same = (got.view(torch.int16) == ref.view(torch.int16)) | nan
    assert bool(same.all()), f'{int((~same).sum())} plane values differ from the round-to-nearest-even chain, first x = {float(x[(~same).any(0)][0])!r}'
    in_range = (x == 0) | ((x.abs() >= SPLIT_LO) & (x.abs() <= SPLIT_HI))
    assert int(in_range.sum()) > 2_000_000
    total = got.double().sum(0)
    exact = total == x.double()
    assert bool(exact[in_range].all()), f'{int((~exact[in_range]).sum())} values in the documented range are not the sum of their planes'
    via_ops = S().ops.split_bf16x3(x[:4096].to(DEV).view(64, 64)).cpu()
    assert via_ops.shape == (3, 64, 64)
    assert bool(((via_ops.view(torch.int16).reshape(3, -1) == ref[:, :4096].view(torch.int16)) | nan[:, :4096]).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# the remaining kernels of rowops.hip (each has its detailed test in test_hip_kernels.py / test_hip_pinned.py): one compact exact check
# each, so that this file alone launches every kernel of the source file
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', [1, 4095, 4096, 4097, 10_000])
def test_partition_slots_is_the_stable_argsort(R):
    """sbr_partition_slots: segment m of the output holds the slots whose modality is m in ascending order, the unused tail of its
    capacity the sentinel R. One launch up to 4,096 slots, histogram + scatter above. Exact."""
    rng = np.random.default_rng(R)
    n_mod = 3
    pos = rng.integers(0, n_mod, size=R).astype(np.int8)
    counts = np.bincount(pos, minlength=n_mod)
    caps = counts + np.array([0, 5, 300])
    offs = np.concatenate([[0], np.cumsum(caps)]).astype(np.int32)
    want = np.full(int(offs[-1]), R, dtype=np.int64)
    for mo in range(n_mod):
        want[offs[mo]:offs[mo] + counts[mo]] = np.flatnonzero(pos == mo)
    pos_d = torch.from_numpy(pos).to(DEV)
    out = torch.full((int(offs[-1]) + 8,), -7, dtype=torch.int32, device=DEV)
    nb = int(_L().lib().sbr_partition_slots_workspace(R))
    ws = torch.zeros(nb // 4 + 8, dtype=torch.int32, device=DEV)
    offs_c = (ctypes.c_int * (n_mod + 1))(*offs.tolist())
    call('sbr_partition_slots', _p(pos_d), R, n_mod, ctypes.cast(offs_c, ctypes.c_void_p), _p(out), _p(ws), nb, stream())
    assert out[:int(offs[-1])].cpu().tolist() == want.tolist() and out[int(offs[-1]):].cpu().tolist() == [-7] * 8


@pytest.mark.parametrize('n,D,xo,xw', [(1, 3, 0, 0), (700, 64, 4, 1), (9000, 130, 0, 2)])
def test_scatter_add_rows_sorted(n, D, xo, xw):
    """The atomic-free lookup gradient from row lists sorted by table row: dW[r] += the rows of r's segment, added in fp32 in sorted order
    and then to dW (m sources: m additions, the last onto the existing value): |err| <= (m + 1) u (|dW| + sum|terms|). (9000, 130): above
    the 1,048,576-element grid cap."""
    n_table, cap = 41, (n + 1) // 2
    rng = np.random.default_rng(n)
    g = _rand(2 * cap, D, seed=31)
    dOut = _Buf(2 * cap, D, D + xo, 0, data=g)
    src = rng.permutation(2 * cap)[:n]
    rows = rng.integers(0, n_table, size=n)
    order = np.argsort(rows, kind='stable')
    perm_d, rs_d = _i64(src[order]), _i32(rows[order])
    dW = _Buf(n_table, D, D + xw, 1, fill=0.5)
    call('sbr_scatter_add_rows_sorted', dOut.ptr, dOut.ld, cap, cap * dOut.ld, _p(perm_d), _p(rs_d), dW.ptr, dW.ld, n, D, stream())
    rt = torch.as_tensor(rows, dtype=torch.int64)
    sg = g[torch.as_tensor(src)].double()
    ref = torch.full((n_table, D), 0.5, dtype=torch.float64).index_add_(0, rt, sg)
    mag = torch.full((n_table, D), 0.5, dtype=torch.float64).index_add_(0, rt, sg.abs())
    m = torch.bincount(rt, minlength=n_table).double()[:, None]
    _assert_bound(dW.check_untouched(None, 'scatter_add_rows_sorted'), ref, (m + 1) * U32 * mag, 'scatter_add_rows_sorted')


@pytest.mark.parametrize('n', [1, 255, 256, 257, 3000])
def test_csr_contains(n):
    """out[j] = 1 iff (rows[j], cols[j]) is stored in the CSR matrix (sorted columns; empty rows, first / last column of a row). Exact."""
    import scipy.sparse as sp
    rng = np.random.default_rng(n)
    mtx = sp.random(30, 200, density=0.1, format='csr', random_state=3)
    mtx.data[:] = 1
    mtx = sp.vstack([mtx, sp.csr_matrix((2, 200))]).tocsr()
    mtx.sort_indices()
    rows, cols = rng.integers(0, 32, size=n), rng.integers(0, 200, size=n)
    r0 = int(np.flatnonzero(np.diff(mtx.indptr) > 1)[0])
    if n >= 3:
        rows[0], cols[0] = r0, mtx.indices[mtx.indptr[r0]]
        rows[1], cols[1] = r0, mtx.indices[mtx.indptr[r0 + 1] - 1]
        rows[2], cols[2] = 31, 0
    ip, ix, r_d, c_d = _i64(mtx.indptr), _i32(mtx.indices), _i64(rows), _i64(cols)
    out = torch.full((n + 8,), 9, dtype=torch.uint8, device=DEV)
    call('sbr_csr_contains', _p(ip), _p(ix), _p(r_d), _p(c_d), n, _p(out), stream())
    want = np.asarray(mtx[rows, cols]).reshape(-1) != 0
    assert out[:n].cpu().tolist() == want.astype(int).tolist() and out[n:].cpu().tolist() == [9] * 8
