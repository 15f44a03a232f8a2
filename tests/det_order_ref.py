"""The order oracle of deterministic mode's fixed-order kernels (csrc/deterministic.hip; colred.h: sbr_col_reduce) and the case lists of
tests/test_hip_det_order.py, with the host rules restated that the cases are derived from. tests/test_det_order_cpu.py asserts on the
CPU that every case reaches the branch it is named for. A plain module: numpy only, no fixtures, no GPU.

The oracle: the segmented row accumulation promises dW[r, :] += the gradient rows of r's sources, added one by one in ASCENDING source
position into an fp32 accumulator that starts at +0, then ONE more fp32 addition onto dW[r, :]. Source rows that are all zero (+0 or -0)
are left out before the grouping; a table row with no source left is not written. There is no multiply, hence nothing to contract, and
the library is built without fast-math: numpy's float32 additions in that order give the kernel's bits exactly."""
import numpy as np

# ---- restated host rules (csrc/deterministic.hip: sbr_det_scatter_add_rows) ------------------------------------------------------
HASH_MULT = 2654435761
MARK_MAX_BLOCKS, ADD_MAX_BLOCKS, WAVES_PER_BLOCK = 4096, 2048, 4
SHORT_MAX = 64                               # segments of up to 64 sources: in-register rank sort; longer ones walk all positions
DET_MAX_D = 512
COLRED_MAX_BLOCKS, COLRED_MAX_C, COLRED_PASSES = 512, 1024, 8


def cdiv(a, b):
    return (a + b - 1) // b


def hash_geometry(n):
    """-> (logH, H): the smallest power of two H >= max(64, 2 n)"""
    logH = 6
    while (1 << logH) < 2 * n:
        logH += 1
    return logH, 1 << logH


def home(r, logH):
    """the home entry of table row r: ((uint32)r * 2654435761) >> (32 - logH)"""
    return ((np.asarray(r, dtype=np.uint64) * np.uint64(HASH_MULT)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - logH)


def probe_table(rows_distinct, n):
    """linear probing of the distinct rows into the table of hash_geometry(n), in the given order (the occupied SET does not depend on
    the order) -> (entry of every row, probes of every row: 1 = landed on its home entry)"""
    logH, H = hash_geometry(n)
    keys = {}
    entry, probes = [], []
    for r in rows_distinct:
        h, k = int(home(r, logH)), 1
        while h in keys:
            h, k = (h + 1) & (H - 1), k + 1
        keys[h] = int(r)
        entry.append(h)
        probes.append(k)
    return np.array(entry), np.array(probes)


def mark_waves(n):
    return min(cdiv(n, WAVES_PER_BLOCK), MARK_MAX_BLOCKS) * WAVES_PER_BLOCK


def add_waves(n):
    return min(cdiv(n, WAVES_PER_BLOCK), ADD_MAX_BLOCKS) * WAVES_PER_BLOCK


def nc_of(D):
    """the 64-column chunks per lane the add kernel is instantiated with"""
    nc = cdiv(D, 64)
    return 1 if nc == 1 else 2 if nc == 2 else 4 if nc <= 4 else 8


def col_reduce_geometry(n, C):
    """colred.h: sbr_col_reduce_blocks and the row ranges of sbr_col_reduce -> (blocks, RL row lanes, chunk rows per block, [(lo, hi)])"""
    RL = 256 // (C >> 2)
    nb = max(1, min(cdiv(n, COLRED_PASSES * RL), COLRED_MAX_BLOCKS))
    chunk = cdiv(n, nb)
    return nb, RL, chunk, [(b * chunk, min(b * chunk + chunk, n)) for b in range(nb)]


def colsum_chain(n, C):
    """the longest fp32 addition chain of one thread of the fixed-slot column sum: its rows lo + rl, lo + rl + RL, ... of a block"""
    nb, RL, chunk, _ = col_reduce_geometry(n, C)
    return cdiv(chunk, RL)


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def _live_sources(g, ii, rows):
    rows = np.asarray(rows)
    src = g[np.asarray(ii)] if ii is not None else g[:len(rows)]
    live = (src != 0).any(axis=1) & (rows >= 0)            # -0.0 != 0 is False, NaN != 0 is True: the kernel's test
    return src, rows, live


def scatter_in_order(g, ii, rows, dW0, order='ascending'):
    """g [n_src, D] fp32, ii (None: identity) and rows [n] -> dW0 with every named row's sources added as the header says. ``order``:
    'descending' and 'chunk_reversed' (positions of one 64-position block in descending order, blocks ascending) are the wrong orders
    the CPU test holds the cases against; the GPU test only uses the default."""
    g, dW0 = np.asarray(g, dtype=np.float32), np.asarray(dW0, dtype=np.float32)
    src, rows, live = _live_sources(g, ii, rows)
    out = dW0.copy()
    pos = np.flatnonzero(live)
    if order == 'descending':
        pos = pos[::-1]
    elif order == 'chunk_reversed':
        pos = pos[np.lexsort((-pos, pos // 64))]
    else:
        assert order == 'ascending'
    acc = {}
    for j in pos:
        r = int(rows[j])
        a = acc.get(r)
        acc[r] = (np.zeros(g.shape[1], dtype=np.float32) if a is None else a) + src[j]
    for r, a in acc.items():
        assert a.dtype == np.float32
        out[r] = dW0[r] + a
    return out


def segment_lengths(g, ii, rows):
    """-> {table row: number of its sources that are not all-zero}"""
    src, rows, live = _live_sources(np.asarray(g, dtype=np.float32), ii, rows)
    r, c = np.unique(rows[live], return_counts=True)
    return dict(zip(r.tolist(), c.tolist()))


# ---- the cases of the segmented scatter ------------------------------------------------------------------------------------------
LADDER = (1, 2, 3, 4, 5, 7, 8, 33, 63, 64, 65, 66, 127, 128, 129, 200)
LADDER_SMALL = (3, 64, 65)
D_EDGES = (1, 63, 64, 65, 128, 192, 256, 257, 512)
NC_WANTED = {1: 1, 63: 1, 64: 1, 65: 2, 128: 2, 192: 4, 256: 4, 257: 8, 512: 8}
GRID_N, GRID_TABLE = 20_011, 12_000
HASH_TABLE_ROWS, HASH_N = 200_000, 300


def wide_values(rng, n, D):
    """randn * 2^randint(-12, 12) per element: partial sums lose different low bits in different orders"""
    return (rng.standard_normal((n, D)) * np.exp2(rng.integers(-12, 13, size=(n, D)))).astype(np.float32)


def prefill(rng, n_table, D):
    """random nonzero dW with some -0.0 entries (a row that nothing live names must keep them)"""
    w = wide_values(rng, n_table, D)
    w[w == 0] = 1.0
    w[rng.random((n_table, D)) < 0.05] = -0.0
    return w


class Case:
    """g [n_src, D], ii ([n] or None), rows [n], dW0 [n_table, D]; ``ladder``: {table row: its exact number of live sources}"""

    def __init__(self, name, g, ii, rows, dW0, ladder=None):
        self.name, self.g, self.ii, self.rows, self.dW0, self.ladder = name, g, ii, np.asarray(rows, dtype=np.int64), dW0, ladder or {}
        self.n, self.D, self.n_table = len(self.rows), g.shape[1], dW0.shape[0]

    def oracle(self, order='ascending'):
        return scatter_in_order(self.g, self.ii, self.rows, self.dW0, order)


def _ladder(name, lengths, D, n_fill, use_ii, seed):
    """table row q gets exactly lengths[q] sources at random positions; n_fill more positions go to rows behind the ladder, two each"""
    rng = np.random.default_rng(seed)
    n = sum(lengths) + n_fill
    rows = np.concatenate([np.full(L, q) for q, L in enumerate(lengths)] + [len(lengths) + np.arange(n_fill) // 2])
    rows = rows[rng.permutation(n)]
    n_table = len(lengths) + cdiv(n_fill, 2) + 3               # the last three rows: named by nobody
    n_src = n + 5 if use_ii else n
    g = wide_values(rng, n_src, D)
    g[(g == 0).all(axis=1)] = 1.0                              # every source row is live: the ladder's lengths are exact
    ii = rng.permutation(n_src)[:n] if use_ii else None
    return Case(name, g, ii, rows, prefill(rng, n_table, D), {q: L for q, L in enumerate(lengths)})


def ladder_case(use_ii=True):
    return _ladder('ladder' if use_ii else 'ladder_null_idx', LADDER, 128, 1500 - sum(LADDER), use_ii, 11 if use_ii else 12)


def d_edge_case(D):
    return _ladder(f'd_edge_{D}', LADDER_SMALL, D, 300 - sum(LADDER_SMALL), True, 100 + D)


def grid_stride_case():
    """more positions than the mark kernel has waves, more segments than the add kernel has waves"""
    rng = np.random.default_rng(21)
    rows = np.concatenate([rng.permutation(GRID_TABLE), rng.integers(0, GRID_TABLE, size=GRID_N - GRID_TABLE)])
    g = wide_values(rng, GRID_N + 5, 64)
    g[(g == 0).all(axis=1)] = 1.0
    return Case('grid_stride', g, rng.permutation(GRID_N + 5)[:GRID_N], rows, prefill(rng, GRID_TABLE, 64))


def _rows_with_home(logH, wanted, count, taken=()):
    """the first ``count`` table rows below HASH_TABLE_ROWS whose home entry is in ``wanted``"""
    r = np.arange(HASH_TABLE_ROWS)
    hit = r[np.isin(home(r, logH), wanted) & ~np.isin(r, taken)]
    assert len(hit) >= count
    return hit[:count]


def _hash_case(name, n, homes_of, count, seed):
    rng = np.random.default_rng(seed)
    logH, H = hash_geometry(n)
    special = _rows_with_home(logH, homes_of(H), count)
    n_table = int(special.max()) + 1
    rows = rng.integers(0, n_table, size=n)
    rows[rng.permutation(n)[:3 * count]] = np.tile(special, 3)      # every special row three times: segments, not single rows
    g = wide_values(rng, n + 5, 64)
    g[(g == 0).all(axis=1)] = 1.0
    c = Case(name, g, rng.permutation(n + 5)[:n], rows, prefill(rng, n_table, 64))
    c.special = special
    return c


def hash_chain_case():
    """12 table rows that share ONE home entry: the last of them to arrive probes past the other eleven"""
    return _hash_case('hash_chain', HASH_N, lambda H: [int(home(7, hash_geometry(HASH_N)[0]))], 12, 31)


def hash_wrap_case():
    """6 table rows whose home entry is H - 1 or H - 2: from the third on they wrap to entry 0"""
    return _hash_case('hash_wrap', HASH_N, lambda H: [H - 1, H - 2], 6, 32)


ZERO_ONLY_ROW = 5


def zero_rows_case():
    """the 'sentinel' construction of tests/test_hip_deterministic.py (770 slots name one table row through ONE zero gradient row, among
    ordinary rows), and table row ZERO_ONLY_ROW named only by zero rows and -0.0 rows, its prefilled row holding a -0.0"""
    rng = np.random.default_rng(41)
    n, n_table, D = 1500, 400, 128
    rows = rng.integers(0, n_table, size=n)
    rows[rows == ZERO_ONLY_ROW] = ZERO_ONLY_ROW + 1
    g = wide_values(rng, n + 3, D)
    g[(g == 0).all(axis=1)] = 1.0
    g[n], g[n + 1], g[n + 2] = 0.0, -0.0, 0.0
    g[n + 2, ::2] = -0.0                                            # a mixed +0 / -0 row is a zero row too
    ii = rng.permutation(n)
    pads = rng.choice(n, size=770 + 9, replace=False)
    ii[pads[:770]] = n
    rows[pads[:770]] = 17
    ii[pads[770:]] = np.tile([n, n + 1, n + 2], 3)
    rows[pads[770:]] = ZERO_ONLY_ROW
    dW0 = prefill(rng, n_table, D)
    dW0[ZERO_ONLY_ROW, :4] = [-0.0, 1.5, -0.0, -2.0]
    return Case('zero_rows', g, ii, rows, dW0)


def single_case():
    rng = np.random.default_rng(51)
    return Case('single', wide_values(rng, 1, 128) + 1.0, None, [2], prefill(rng, 4, 128), {2: 1})


def scatter_cases():
    return ([ladder_case(True), ladder_case(False)] + [d_edge_case(D) for D in D_EDGES]
            + [grid_stride_case(), hash_chain_case(), hash_wrap_case(), zero_rows_case(), single_case()])


SCATTER_CASE_NAMES = (['ladder', 'ladder_null_idx'] + [f'd_edge_{D}' for D in D_EDGES]
                      + ['grid_stride', 'hash_chain', 'hash_wrap', 'zero_rows', 'single'])
_CACHE = {}


def scatter_case(name):
    """cases and their oracles are built once and shared (callers must not modify them)"""
    if not _CACHE:
        for c in scatter_cases():
            _CACHE[c.name] = c
        assert list(_CACHE) == SCATTER_CASE_NAMES
    return _CACHE[name]


# ---- the cases of the fixed-slot column sum: (n, C, ld - C) -----------------------------------------------------------------------
COLSUM_CASES = ((1, 4, 0), (2049, 4, 4), (4097, 1024, 0), (520, 1024, 4), (1777, 260, 8), (90_112, 128, 0))
COLSUM_EMPTY_TAIL = (4097, 1024)             # capped at 512 blocks of 9 rows: the blocks from 456 on have no row
COLSUM_STALE = (8192, 1024)                  # run right before it with all values 1e6: all 512 slots hold large sums
