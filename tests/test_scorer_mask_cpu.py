"""CPU: the oracle and the constructions of the fused scorers' exclusion-mask tests (tests/scorer_mask_cases.py). The GPU test
(tests/test_hip_scorer_mask.py) compares bit for bit against what is pinned here: that the integer scores are exact in both operand
formats, that the rotation observes every item once, that ``expected_lists`` is the plain per-user ranking, and that every pattern really
has the group counts, row kinds and tile placements it is named after (a pattern that drifted would pass vacuously)."""
import math

import numpy as np
import pytest
import torch

import scorer_mask_cases as C

SIZES = (1, 2, 31, 63, 64, 65, 100, 129, 200, 3073, 6145, 8192, 65536)


def _bf16_rne(x):
    b = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


@pytest.mark.parametrize('I', SIZES)
def test_integer_scores_are_exact_in_fp16_and_in_the_three_plane_bf16_split(I):
    for a in (1, C.stride(I)):
        rk = C.ranks(I, 10, 3, a)
        assert sorted(rk.tolist()) == list(range(I))
        u, it = C.operands(I, 64, rk, Bu=2)
        s = C.scores(I, rk)
        assert u.dtype == np.float32 and it.dtype == np.float32 and sorted(s.tolist()) == list(range(I))
        # fp16: the operands survive the round trip, products with 1.0 and their fp32 sum are the integer
        h = torch.from_numpy(it).half()
        assert torch.equal(h.float(), torch.from_numpy(it)) and torch.equal(torch.from_numpy(u).half().float(), torch.from_numpy(u))
        got = torch.from_numpy(u).half().float() @ h.float().t()
        assert np.array_equal(got.numpy(), np.broadcast_to(s.astype(np.float32), (2, I)))
        # bf16 split: three planes, round to nearest even of the remainder each, sum to the value exactly
        p1 = _bf16_rne(it)
        p2 = _bf16_rne(it - p1)
        p3 = _bf16_rne(it - p1 - p2)
        assert np.array_equal(p1 + p2 + p3, it) and np.array_equal(((p1 + p2 + p3) @ u.T)[:, 0], s.astype(np.float32))
        assert float(s.max()) < 2 ** 24


@pytest.mark.parametrize('I,k', [(1, 1), (1, 33), (63, 10), (64, 32), (65, 1), (100, 33), (129, 10), (200, 1), (200, 10), (200, 32),
                                 (200, 33), (200, 128), (33, 128), (300, 10)])
def test_every_item_is_in_exactly_one_window_over_the_rounds(I, k):
    for a in (1, C.stride(I)):
        assert a == 1 or (a > 64 and math.gcd(a, I) == 1)
        seen = np.zeros(I, dtype=np.int64)
        for r in range(C.n_rounds(I, k)):
            win = C.window(I, k, r, a)
            assert (C.ranks(I, k, r, a)[win] < k).all()              # inside the unexcluded top-k window of its round
            seen[win] += 1
        assert (seen == 1).all(), f'I={I} k={k} a={a}: {seen.tolist()}'
    if I >= 130:                                                     # the strided window is spread over the tiles, a = 1 is not
        assert len(set(C.window(I, 10, 1, C.stride(I)) // 64)) >= 3 and len(set(C.window(I, 10, 1, 1) // 64)) <= 2
        assert (np.diff(np.argsort(C.ranks(I, 10, 1, C.stride(I)))[:10]) % I > 64).all()       # consecutive ranks: more than a tile apart


def test_expected_lists_equal_a_brute_force_ranking():
    rng = np.random.default_rng(0)
    for (Bu, I, k, off) in ((7, 50, 10, 0), (5, 20, 33, 300), (3, 1, 4, 9), (6, 40, 40, 1)):
        sc = rng.permutation(I)
        sc[: I // 3] = sc[0]                                         # ties: ascending index decides
        mask = rng.random((Bu, I)) < 0.4
        mask[0], mask[-1] = True, False
        val, idx = C.expected_lists(sc, mask, k, off)
        assert val.dtype == np.float32 and idx.dtype == np.int32 and val.shape == idx.shape == (Bu, k)
        for u in range(Bu):
            items = sorted((j for j in range(I) if not mask[u, j]), key=lambda j: (-sc[j], j))[:k]
            want_i = [j + off for j in items] + [-1] * (k - len(items))
            want_v = [float(sc[j]) for j in items] + [-math.inf] * (k - len(items))
            assert idx[u].tolist() == want_i and val[u].tolist() == want_v
        win = np.arange(I)
        assert np.array_equal(C.observed_mask(C.expected_lists(sc, mask, I, off)[1], win, off), mask)


def _rows_sorted_unique(m):
    for u in range(m.shape[0]):
        r = m.indices[m.indptr[u]:m.indptr[u + 1]]
        assert (np.diff(r) > 0).all()


@pytest.mark.parametrize('Bu', sorted(C.QUAD_COUNTS))
def test_quad_edge_pattern_has_the_group_counts_it_claims(Bu):
    c = C.quad_edges(Bu)
    _rows_sorted_unique(c.csr)
    assert C.group_counts(c).tolist() == list(C.QUAD_COUNTS[Bu]) and len(C.QUAD_COUNTS[Bu]) == -(-Bu // 32)
    cols = C.three_tile_cols(8192, 64)
    assert len(cols) == 12 and {c // 64 for c in cols} == {0, 64, 127}
    c2 = C.quad_edges(Bu, I=8192, cols=cols)
    assert C.group_counts(c2).tolist() == list(C.QUAD_COUNTS[Bu]) and set(c2.csr.indices) <= set(cols)


def test_quad_edge_patterns_cover_every_count_around_a_quad_an_empty_middle_group_and_ragged_groups():
    assert {n for v in C.QUAD_COUNTS.values() for n in v} == {0, 1, 3, 4, 5, 7, 8, 9}
    assert C.QUAD_COUNTS[96][1] == 0 and C.QUAD_COUNTS[96][0] > 0 and C.QUAD_COUNTS[96][2] > 0
    assert {1, 31, 32, 33, 65} <= set(C.QUAD_COUNTS)


@pytest.mark.parametrize('T', [64, 32])
def test_full_tile_pattern(T):
    c = C.full_tile(T)
    _rows_sorted_unique(c.csr)
    m = C.dense_mask(c)
    assert c.I == 3 * T and m[:32, T:2 * T].all() and not m[:32, :T].any() and not m[:32, 2 * T:].any()
    assert m[32].all() and C.group_counts(c).tolist() == [32 * T, 3 * T, 1]
    assert C.expected_lists(np.arange(c.I), m, 5)[1][32].tolist() == [-1] * 5


@pytest.mark.parametrize('T', [64, 32])
def test_tile_edge_patterns(T):
    assert len(C.TILE_EDGE_I[T]) == 6 and {1, T - 1, T, T + 1, 2 * T + 1} <= set(C.TILE_EDGE_I[T])
    for I in C.TILE_EDGE_I[T]:
        c = C.tile_edges(T, I)
        _rows_sorted_unique(c.csr)
        m = C.dense_mask(c)
        assert c.edge == sorted({x for x in (0, T - 1, T, 2 * T - 1, I - 1) if x < I}) and I - 1 in c.edge and 0 in c.edge
        assert not np.delete(m, c.edge, axis=1).any()
        subsets = {tuple(row) for row in m[:, c.edge]}
        assert len(subsets) == 2 ** len(c.edge)                      # every combination of the edge columns, the empty one included


def test_shard_clipping_pattern_has_the_nine_row_kinds():
    for (off, I) in ((300, 200), (250, 200), (300, 8192)):
        c = C.shard_clip(off=off, I=I)
        _rows_sorted_unique(c.csr)
        end = off + I
        assert c.csr.shape[1] == (1000 if I == 200 and off == 300 else c.csr.shape[1]) and set(c.kinds) == set(C.CLIP_KINDS)
        for u, kind in enumerate(c.kinds):
            r = c.csr.indices[c.csr.indptr[u]:c.csr.indptr[u + 1]]
            inside = r[(r >= off) & (r < end)]
            ok = {
                'below': len(r) > 0 and r[-1] < off - 1,
                'above': len(r) > 0 and r[0] > end,
                'last_at_off_minus_1': len(r) > 0 and r[-1] == off - 1,
                'first_at_off': len(r) > 0 and r[0] == off,
                'last_at_end_minus_1': len(r) > 0 and r[-1] == end - 1 and r[0] < off,
                'first_at_end': len(r) > 0 and r[0] == end,
                'spanning': len(r) > 0 and r[0] < off and r[-1] >= end and {off - 1, off, end - 1, end} <= set(r.tolist()),
                'empty': len(r) == 0,
                'whole': len(r) == c.csr.shape[1],
            }[kind]
            assert ok, (u, kind, r[:8])
            assert len(inside) == C.in_shard_counts(c)[u]
            if kind in ('below', 'above', 'last_at_off_minus_1', 'first_at_end', 'empty'):
                assert len(inside) == 0
    a = C.shard_clip(off=300)
    b = C.reshard(a, 250)
    assert b.csr is a.csr and b.item_offset == 250
    assert not np.array_equal(C.dense_mask(a), C.dense_mask(b))      # another offset is another mask


def test_user_index_map_patterns():
    for repeat in (False, True):
        c = C.u_idx_map(repeat)
        _rows_sorted_unique(c.csr)
        assert c.csr.shape == (300, 200) and c.Bu == 70
        assert len(set(c.u_idx.tolist())) == (62 if repeat else 70)
        assert (np.diff(c.u_idx[:35]) == -1).all() and not (np.diff(c.u_idx[35:]) > 0).all() and not (np.diff(c.u_idx[35:]) < 0).all()
        assert C.in_shard_counts(c).sum() <= c.csr.nnz
        # a mix-up of scored row and CSR row would show: the mapped rows differ from the rows of the same position
        assert not np.array_equal(C.dense_mask(c), np.asarray(c.csr[np.arange(70)].toarray() != 0))
        assert (np.diff(c.csr.indptr) == 0).any()


@pytest.mark.parametrize('key', sorted(C.PREFIX_I))
def test_prefix_pattern(key):
    T, pre = key
    sizes = C.PREFIX_I[key]
    first = (6 * pre - 1) * T + 1                                    # smallest catalogue of 6 * pre tiles
    assert sizes == (first - 1, first, 6 * pre * T, 6 * pre * T + 1)
    assert [-(-I // T) >= 6 * pre for I in sizes] == [False, True, True, True]
    for I in sizes:
        c = C.prefix(I, T, pre)
        _rows_sorted_unique(c.csr)
        m = C.dense_mask(c)
        assert c.Bu == 40 and m[0, :40].all() and not m[1].any()
        assert len({tuple(r) for r in m[:, :40]}) == 40            # every user another subset of the top 40
        assert (np.flatnonzero(C.ranks(I, 20, 0, 1) < 40) < pre * T).all()
        assert m[2, pre * T - 1] and m[3, pre * T] and m[4, I - 1] and m[5, [pre * T - 1, pre * T, I - 1]].all()
        # the excluded scores are among those a class maximum would count: user 0's list starts behind them
        assert C.expected_lists(C.scores(I, C.ranks(I, 20, 0, 1)), m, 20)[1][0].tolist() == list(range(40, 60))


@pytest.mark.parametrize('G,T', [(256, 64), (256, 32), (304, 64), (8, 32)])
def test_partial_wave_pattern(G, T):
    c = C.partial_wave(G, T)
    _rows_sorted_unique(c.csr)
    m = C.dense_mask(c)
    n_tiles = -(-c.I // T)
    assert c.Bu == 32 * (G + 1) and c.I == 300
    last = m[32 * G:]
    for t in range(n_tiles):
        assert (last[:, t * T:(t + 1) * T].sum(1) == 1).all()        # every user of the remainder unit, every tile
    gc = C.group_counts(c)
    assert gc[G] == 32 * n_tiles and set(np.flatnonzero(gc).tolist()) == {0, 1, G // 2, G - 1, G}
