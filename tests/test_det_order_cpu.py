"""The CPU side of tests/test_hip_det_order.py: every case of tests/det_order_ref.py meets the precondition under which its GPU test
proves what it is named for — the order oracle is order SENSITIVE on the ladder rows, and each reach case really reaches its branch
under the restated host rules (segment lengths on both sides of 64, probe chains, the wrap to entry 0, second trips of both capped
grids, empty trailing blocks of the column sum, the NC instantiations)."""
import numpy as np
import pytest

import det_order_ref as R


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def test_the_oracle_adds_in_ascending_position_and_leaves_unnamed_rows_alone():
    """a hand-made case: (2^24 + 1) + 1 in fp32 depends on the order; zero rows, -0.0 rows and negative destinations are left out"""
    big = np.float32(2.0 ** 24)
    g = np.array([[big, 1.0], [1.0, 1.0], [1.0, 1.0], [0.0, -0.0], [-0.0, -0.0], [5.0, 5.0]], dtype=np.float32)
    dW0 = np.array([[-0.0, 3.0], [-0.0, 7.0], [-0.0, -0.0]], dtype=np.float32)
    rows = np.array([0, 0, 0, 1, 1, -1])
    out = R.scatter_in_order(g, None, rows, dW0)
    assert out[0].tolist() == [2.0 ** 24, 6.0]                       # ((2^24 + 1) + 1) = 2^24: each 1 is rounded away
    assert R.scatter_in_order(g, None, rows, dW0, 'descending')[0].tolist() == [2.0 ** 24 + 2, 6.0]
    assert (_bits(out[1:]) == _bits(dW0[1:])).all(), 'a row named only by zero rows, or by nobody, must keep its bits (-0.0 included)'
    ii = np.array([2, 1, 0, 3, 4, 5])
    assert R.scatter_in_order(g, ii, rows, dW0)[0].tolist() == [2.0 ** 24 + 2, 6.0]      # in_idx decides the value, not the position
    nan = np.array([[np.nan, 0.0]], dtype=np.float32)
    assert np.isnan(R.scatter_in_order(nan, None, [2], dW0)[2, 0]), 'a NaN row counts as nonzero'
    assert R.segment_lengths(g, None, rows) == {0: 3}


def test_restated_geometry():
    assert R.hash_geometry(1) == (6, 64) and R.hash_geometry(32) == (6, 64) and R.hash_geometry(33) == (7, 128)
    assert R.hash_geometry(300) == (10, 1024) and R.hash_geometry(R.GRID_N) == (16, 65536)
    assert int(R.home(1, 10)) == (2654435761 >> 22) and int(R.home(3, 6)) == ((3 * 2654435761) & 0xFFFFFFFF) >> 26
    assert R.mark_waves(16_384) == 16_384 == R.mark_waves(10 ** 6) and R.add_waves(8192) == 8192 == R.add_waves(10 ** 6)
    assert R.col_reduce_geometry(90_112, 128)[:3] == (512, 8, 176) and R.col_reduce_geometry(1, 4)[:3] == (1, 256, 1)


@pytest.mark.parametrize('name', [n for n in R.SCATTER_CASE_NAMES if n.startswith(('ladder', 'd_edge'))])
def test_ladder_rows_have_their_lengths_and_are_order_sensitive(name):
    """every ladder row has exactly its L live sources; for L >= 3 the ascending sum differs in bits from the descending one in at least
    one column (else a flipped rank comparison would pass), and for L > 64 from the sum that reverses every 64-position block (the long
    path's list index). L = 2 cannot differ: fp32 addition commutes."""
    c = R.scatter_case(name)
    want = R.LADDER if name.startswith('ladder') else R.LADDER_SMALL
    assert tuple(c.ladder.values()) == want and c.D == (128 if name.startswith('ladder') else int(name.rsplit('_', 1)[1]))
    assert (c.ii is None) == (name == 'ladder_null_idx')
    lens = R.segment_lengths(c.g, c.ii, c.rows)
    assert all(lens[r] == L for r, L in c.ladder.items())
    assert {L for L in want if L <= R.SHORT_MAX} and {L for L in want if L > R.SHORT_MAX}, 'both paths of the add kernel'
    if name.startswith('ladder'):
        assert {63, 64, 65} <= set(want) and abs(c.n - 1500) <= 0
    else:
        assert c.n == 300
    asc, desc, rev = c.oracle(), c.oracle('descending'), c.oracle('chunk_reversed')
    for r, L in c.ladder.items():
        if L >= 3:
            assert (_bits(asc[r]) != _bits(desc[r])).any(), f'{name}: the row of L = {L} has the same bits in descending order'
        if L > R.SHORT_MAX:
            assert (_bits(asc[r]) != _bits(rev[r])).any(), f'{name}: the row of L = {L} has the same bits with its blocks reversed'
    untouched = np.setdiff1d(np.arange(c.n_table), np.unique(c.rows))
    assert len(untouched) >= 3 and (_bits(asc[untouched]) == _bits(c.dW0[untouched])).all()
    assert (c.dW0 != 0).mean() > 0.9 and (_bits(c.dW0) == np.int32(-2 ** 31)).any(), 'the prefill is nonzero and holds -0.0'
    plain = R.scatter_in_order(c.g, c.ii, c.rows, np.zeros_like(c.dW0))
    assert all((_bits(asc[r]) != _bits(plain[r])).any() for r in c.ladder), '+= and = must differ on every ladder row'


def test_d_edges_map_to_every_instantiation():
    assert {D: R.nc_of(D) for D in R.D_EDGES} == R.NC_WANTED and set(R.NC_WANTED.values()) == {1, 2, 4, 8}
    assert R.nc_of(R.DET_MAX_D) == 8 and R.cdiv(R.DET_MAX_D + 1, 64) == 9           # 513: a ninth chunk no instantiation has


def test_grid_stride_case_takes_both_loops_twice():
    c = R.scatter_case('grid_stride')
    assert c.n == 20_011 and c.n_table == 12_000 and c.D == 64
    assert c.n > R.mark_waves(c.n) == 16_384, 'the mark kernel needs a second trip'
    lens = R.segment_lengths(c.g, c.ii, c.rows)
    assert len(lens) == 12_000 > R.add_waves(c.n) == 8192, 'the add kernel needs a second trip'
    assert sorted(c.rows[:12_000].tolist()) == list(range(12_000))


def test_hash_cases_probe_and_wrap():
    logH, H = R.hash_geometry(R.HASH_N)
    for name in ('hash_chain', 'hash_wrap'):
        c = R.scatter_case(name)
        assert c.n == R.HASH_N and c.n_table <= R.HASH_TABLE_ROWS and c.D == 64
        lens = R.segment_lengths(c.g, c.ii, c.rows)
        assert all(lens[int(r)] >= 3 for r in c.special)
        distinct = np.array(sorted(lens))
        entry, probes = R.probe_table(distinct, c.n)
        assert len(set(entry.tolist())) == len(distinct) <= c.n and entry.max() < H
        sp = np.isin(distinct, c.special)
        if name == 'hash_chain':
            assert len(c.special) >= 8 and len(set(R.home(c.special, logH).tolist())) == 1
            assert probes[sp].max() >= 8, 'no probe chain of 8 entries'
            for order in (distinct[::-1], np.random.default_rng(0).permutation(distinct)):      # whatever the arrival order
                assert R.probe_table(order, c.n)[1].max() >= 8
        else:
            homes = R.home(c.special, logH)
            assert len(set(c.special.tolist())) >= 3 and set(homes.tolist()) <= {H - 1, H - 2}
            assert (entry[sp] < H - 2).any(), 'no special row wrapped to the front of the table'
            assert 0 in entry[sp].tolist() or 0 in entry.tolist()
            for order in (distinct[::-1], np.random.default_rng(0).permutation(distinct)):
                e2 = R.probe_table(order, c.n)[0]
                assert (e2[np.isin(order, c.special)] < H - 2).any()


def test_zero_rows_case():
    c = R.scatter_case('zero_rows')
    src = c.g[c.ii]
    named_by = src[c.rows == R.ZERO_ONLY_ROW]
    assert len(named_by) == 9 and (named_by == 0).all() and np.signbit(named_by).any() and (~np.signbit(named_by)).any()
    assert R.ZERO_ONLY_ROW not in R.segment_lengths(c.g, c.ii, c.rows)
    assert (_bits(c.dW0[R.ZERO_ONLY_ROW, :3:2]) == np.int32(-2 ** 31)).all()
    assert (_bits(c.oracle()[R.ZERO_ONLY_ROW]) == _bits(c.dW0[R.ZERO_ONLY_ROW])).all()
    sentinel = (c.ii == c.n)
    assert int(sentinel.sum()) >= 770 and len(set(c.rows[sentinel].tolist()) - {R.ZERO_ONLY_ROW}) == 1 and (c.g[c.n] == 0).all()


def test_colsum_cases_and_their_empty_blocks():
    assert R.COLSUM_EMPTY_TAIL + (0,) in R.COLSUM_CASES
    nb, RL, chunk, ranges = R.col_reduce_geometry(*R.COLSUM_EMPTY_TAIL)
    assert (nb, RL, chunk) == (512, 1, 9)
    empty = [b for b, (lo, hi) in enumerate(ranges) if lo >= R.COLSUM_EMPTY_TAIL[0]]
    assert empty == list(range(456, 512)), 'the trailing blocks must have an empty row range'
    assert R.col_reduce_geometry(*R.COLSUM_STALE)[0] == 512 and all(hi > lo for lo, hi in R.col_reduce_geometry(*R.COLSUM_STALE)[3])
    for n, C, xl in R.COLSUM_CASES:
        nb, RL, chunk, ranges = R.col_reduce_geometry(n, C)
        assert C % 4 == 0 and 4 <= C <= R.COLRED_MAX_C and (C + xl) % 4 == 0
        assert ranges[0][0] == 0 and max(hi for lo, hi in ranges) == n and sum(max(hi - lo, 0) for lo, hi in ranges) == n
        assert R.colsum_chain(n, C) == R.cdiv(chunk, RL) >= 1
    assert {C for n, C, xl in R.COLSUM_CASES} >= {4, 1024} and {xl for n, C, xl in R.COLSUM_CASES} >= {0, 4, 8}
    assert {R.col_reduce_geometry(n, C)[0] for n, C, xl in R.COLSUM_CASES} >= {1, 512}
    assert R.col_reduce_geometry(1777, 260)[1] == 3 and 3 * 65 < 256, 'C = 260: 61 threads of a block own no row lane'
