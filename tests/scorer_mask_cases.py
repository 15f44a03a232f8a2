"""Cases of the fused scorers' exclusion-mask tests (tests/test_scorer_mask_cpu.py, tests/test_hip_scorer_mask.py): numpy / scipy only,
no GPU, no project imports.

**Scores that are exact integers.** Every user row is (1, 1, 0, ...); item j of rank p(j) in [0, I) is (64 (s // 64), s % 64, 0, ...)
with s = I - 1 - p(j). The score of item j is s for every user: distinct per item and, for I <= 65536, exact in fp16 (multiples of 64
up to 65472, integers below 64, products with 1.0 and their fp32 sum) and in the three-plane bf16 split (integers below 2^24). Lists
therefore compare bit for bit with an integer oracle: no tolerance, no near-ties. All users share the scores; their exclusion rows differ.

**Rotation.** Round r = 0 .. ceil(I / k) - 1 uses the ranks p_r(j) = (a j + r k) mod I; a = 1 keeps the top window contiguous (one or
two tiles), a coprime to I and larger than 64 spreads it over all tiles. An item of rank < k is listed for a user iff it is not masked
for that user (at most k - 1 items outrank it), so a round observes the mask bit of every (user, item of its window). ``window``
returns the part of the top-k window that makes the windows of all rounds a partition of the catalogue.

**Patterns.** Each is a ``Case``: a scipy CSR (sorted, unique rows) over n_users_total x n_items_total, the scored rows ``u_idx``, the
item shard [item_offset, item_offset + I) and the facts the CPU test checks the pattern against."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

QUAD_COUNTS = {96: (4, 0, 9), 1: (1,), 31: (3,), 32: (5,), 33: (7, 1), 65: (8, 4, 9)}      # in-shard events per 32-user group
TILE_EDGE_I = {64: (1, 63, 64, 65, 129, 200), 32: (1, 31, 32, 33, 65, 100)}
CLIP_KINDS = ('below', 'above', 'last_at_off_minus_1', 'first_at_off', 'last_at_end_minus_1', 'first_at_end', 'spanning', 'empty', 'whole')
# (tile width, prefix tiles) -> the catalogues around the prefix pass: the pass runs from 6 * prefix tiles on, i.e. from
# I = (6 * pre - 1) * T + 1; 6 * pre * T and that plus 1 are the sizes where the last of those tiles is full / a new one starts
PREFIX_I = {(64, 16): (6080, 6081, 6144, 6145), (32, 16): (3040, 3041, 3072, 3073), (32, 32): (6112, 6113, 6144, 6145)}


# ---- integer scores ---------------------------------------------------------------------------------------------------------
def n_rounds(I, k):
    return -(-I // k)


@functools.lru_cache(maxsize=None)
def stride(I):
    """an a in (64, 64 + I] coprime to I: the one whose inverse g mod I — the items of ranks p, p + 1 lie g apart — is nearest to
    0.382 I (the golden section: consecutive ranks fall into different tiles, and the top window covers the catalogue evenly)"""
    want = 0.381966 * I
    best = None
    for a in range(65, 65 + I):
        if math.gcd(a, I) == 1:
            g = pow(a, -1, I) if I > 1 else 0
            if best is None or abs(g - want) < best[0]:
                best = (abs(g - want), a)
    return best[1]


def ranks(I, k, r, a):
    return (a * np.arange(I, dtype=np.int64) + r * k) % I


def scores(I, rk):
    return I - 1 - np.asarray(rk, dtype=np.int64)


def operands(I, D, rk, Bu=1):
    """-> (user rows [Bu, D], item rows [I, D]) in fp32"""
    s = scores(I, rk)
    it = np.zeros((I, D), dtype=np.float32)
    it[:, 0] = 64 * (s // 64)
    it[:, 1] = s % 64
    u = np.zeros((Bu, D), dtype=np.float32)
    u[:, :2] = 1.0
    return u, it


def window(I, k, r, a):
    """items observed by round r: rank < k, round 0 cut to the ranks the later rounds do not wrap onto — over all rounds a partition"""
    rk = ranks(I, k, r, a)
    w = min(k, I)
    if r == 0:
        w = min(w, I - (n_rounds(I, k) - 1) * k)
    return np.flatnonzero(rk < w)


# ---- oracle -----------------------------------------------------------------------------------------------------------------
def expected_lists(sc, dense_mask, k, item_offset=0):
    """-> (val float32 [Bu, k], idx int32 [Bu, k]): the non-excluded items of the shard by (score desc, index asc), global indices,
    (-inf, -1) behind fewer than k of them"""
    sc = np.asarray(sc)
    Bu, I = dense_mask.shape
    order = np.lexsort((np.arange(I), -sc))
    m = dense_mask[:, order]
    pos = np.argsort(m, axis=1, kind='stable')[:, :k]                  # non-excluded first, in `order`
    n_ok = (~m).sum(1)
    cols = order[pos]
    valid = np.arange(pos.shape[1])[None, :] < n_ok[:, None]
    val = np.full((Bu, k), -np.inf, dtype=np.float32)
    idx = np.full((Bu, k), -1, dtype=np.int32)
    val[:, :pos.shape[1]] = np.where(valid, sc[cols].astype(np.float32), -np.inf)
    idx[:, :pos.shape[1]] = np.where(valid, cols + item_offset, -1)
    return val, idx


def observed_mask(idx, win, item_offset=0):
    """the mask bits a round's lists show for the items of its window: bool [Bu, len(win)], True = not listed = masked"""
    listed = (idx[:, :, None] == (np.asarray(win) + item_offset)[None, None, :]).any(1)
    return ~listed


# ---- patterns ---------------------------------------------------------------------------------------------------------------
def _csr(rows, cols, shape):
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    m = sp.csr_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=shape)
    assert m.nnz == len(rows), 'duplicate (user, item)'
    m.sort_indices()
    return m


def _case(name, m, u_idx, item_offset, I, **facts):
    u_idx = np.asarray(u_idx, dtype=np.int64)
    c = SimpleNamespace(name=name, csr=m, u_idx=u_idx, item_offset=int(item_offset), I=int(I), Bu=len(u_idx), **facts)
    # the C interface's precondition: the in-shard entries of the scored rows, counted per repetition, fit into excl_nnz = csr.nnz
    assert in_shard_counts(c).sum() <= max(m.nnz, 0), f'{name}: the scored rows hold more in-shard exclusions than the CSR has entries'
    return c


def dense_mask(c):
    return np.asarray(c.csr[c.u_idx][:, c.item_offset:c.item_offset + c.I].toarray() != 0)


def in_shard_counts(c):
    """in-shard exclusions of every scored row (a repeated row counts once per repetition)"""
    return dense_mask(c).sum(1)


def group_counts(c):
    n = in_shard_counts(c)
    return np.add.reduceat(n, np.arange(0, c.Bu, 32))


def quad_edges(Bu, I=200, cols=None, seed=0):
    """per 32-user group QUAD_COUNTS[Bu] events at random (user of the group, item) pairs; ``cols``: the item columns to draw from"""
    rng = np.random.default_rng(1000 + Bu + seed)
    cols = np.arange(I) if cols is None else np.asarray(cols)
    rows_, cols_ = [], []
    for g, n in enumerate(QUAD_COUNTS[Bu]):
        n_u = min(32, Bu - 32 * g)
        flat = rng.choice(n_u * len(cols), size=n, replace=False)
        rows_ += list(32 * g + flat // len(cols))
        cols_ += list(cols[flat % len(cols)])
    return _case(f'quad-Bu{Bu}', _csr(rows_, cols_, (Bu, I)), np.arange(Bu), 0, I, counts=QUAD_COUNTS[Bu])


def three_tile_cols(I, T):
    """twelve columns at the edges of the first, a middle and the last tile of a large catalogue"""
    mid = (-(-I // T) // 2) * T
    return [0, 1, 2, T - 1, mid, mid + 1, mid + 5, mid + T - 1, I - T, I - 3, I - 2, I - 1]


def reshard(c, item_offset, I=None):
    """the same CSR and scored rows, another item shard"""
    return _case(f'{c.name}-off{item_offset}', c.csr, c.u_idx, item_offset, c.I if I is None else I)


def full_tile(T):
    """group 0: every user excludes all of tile 1 (32 T events, tiles 0 and 2 untouched); group 1: user 32 excludes the whole shard;
    group 2 (ragged): one event"""
    I, Bu = 3 * T, 70
    rows_ = list(np.repeat(np.arange(32), T)) + [32] * I + [66]
    cols_ = list(np.tile(np.arange(T, 2 * T), 32)) + list(range(I)) + [2 * T + 1]
    return _case(f'fulltile-T{T}', _csr(rows_, cols_, (Bu, I)), np.arange(Bu), 0, I, T=T)


def tile_edge_cols(T, I):
    return sorted({c for c in (0, T - 1, T, 2 * T - 1, I - 1) if 0 <= c < I})


def tile_edges(T, I, Bu=40):
    """user u excludes the subset of the edge columns {0, T-1, T, 2T-1, I-1} that the bits of u name: every subset occurs"""
    edge = tile_edge_cols(T, I)
    rows_, cols_ = [], []
    for u in range(Bu):
        for b, c in enumerate(edge):
            if (u >> b) & 1:
                rows_.append(u)
                cols_.append(c)
    return _case(f'edges-T{T}-I{I}', _csr(rows_, cols_, (Bu, I)), np.arange(Bu), 0, I, T=T, edge=edge)


def shard_clip(off=300, I=200, above=500, Bu=45):
    """rows of the nine CLIP_KINDS (user u is of kind u % 9, variant v = u // 9) around the shard [off, off + I) of a catalogue of
    off + I + above items"""
    end, total = off + I, off + I + above
    mid = off + I // 2
    rows_, cols_ = [], []
    for u in range(Bu):
        v = u // 9
        row = {
            'below': [3 + v, off // 2, off - 10],
            'above': [end + 10 + v, end + above // 2, total - 1],
            'last_at_off_minus_1': [10 + v, off - 1],
            'first_at_off': [off, mid + 20 + v, end + 100],
            'last_at_end_minus_1': [off // 3, off + 10 + v, end - 1],
            'first_at_end': [end, end + 200 + v],
            'spanning': [50, off - 1, off, off + 1 + v, mid, end - 1, end, total - 100],
            'empty': [],
            'whole': list(range(total)),
        }[CLIP_KINDS[u % 9]]
        rows_ += [u] * len(row)
        cols_ += row
    return _case(f'clip-off{off}-I{I}', _csr(rows_, cols_, (Bu, total)), np.arange(Bu), off, I, kinds=[CLIP_KINDS[u % 9] for u in range(Bu)])


def u_idx_map(repeat=False, n_users_total=300, I=200, n_scored=70, seed=7):
    """70 of the CSR's 300 users: a descending run, then shuffled picks; ``repeat``: 8 of them occur twice"""
    rng = np.random.default_rng(seed)
    n_per = rng.integers(0, 9, size=n_users_total)
    rows_, cols_ = [], []
    for u in range(n_users_total):
        rows_ += [u] * int(n_per[u])
        cols_ += list(rng.choice(I, size=int(n_per[u]), replace=False))
    half = n_scored // 2
    head = np.arange(n_users_total - 1, n_users_total - 1 - half, -1)
    tail = rng.permutation(n_users_total - half)[:n_scored - half]
    u_idx = np.concatenate([head, tail])
    if repeat:
        u_idx[-8:] = u_idx[3:11]
    return _case(f'uidx-{"repeat" if repeat else "distinct"}', _csr(rows_, cols_, (n_users_total, I)), u_idx, 0, I)


def prefix(I, T, pre_tiles, Bu=40, top=40, seed=3):
    """every user excludes another subset of the ``top`` best items of round (a = 1, r = 0) — items 0 .. top - 1, inside the prefix
    tiles —: user 0 all of them, user 1 none; plus exclusions at the prefix pass's last column, the first behind it and the last item"""
    rng = np.random.default_rng(seed + I)
    sub = rng.random((Bu, top)) < 0.5
    sub[0], sub[1] = True, False
    rows_, cols_ = [list(x) for x in np.nonzero(sub)]
    for u, c in ((2, pre_tiles * T - 1), (3, pre_tiles * T), (4, I - 1), (5, pre_tiles * T - 1), (5, pre_tiles * T), (5, I - 1)):
        rows_.append(u)
        cols_.append(c)
    return _case(f'prefix-I{I}-T{T}', _csr(rows_, cols_, (Bu, I)), np.arange(Bu), 0, I, T=T, pre_tiles=pre_tiles, top=top)


def partial_wave(G, T, I=300):
    """Bu = 32 (G + 1): G + 1 units on G compute units = one full wave everywhere + ONE remainder unit cut into parts by item tile. Every
    user of that last unit has an exclusion in every tile; units 0, 1, G // 2 and G - 1 have a few"""
    Bu = 32 * (G + 1)
    n_tiles = -(-I // T)
    rows_, cols_ = [], []
    for u in range(32 * G, Bu):
        for t in range(n_tiles):
            width = min(T, I - t * T)
            rows_.append(u)
            cols_.append(t * T + (5 * u + 3 * t) % width)
    for unit in sorted({0, 1, G // 2, G - 1}):
        for e in range(5):
            rows_.append(32 * unit + (7 * e + unit) % 32)
            cols_.append((61 * e + 13 * unit) % I)
    return _case(f'partial-G{G}-T{T}', _csr(rows_, cols_, (Bu, I)), np.arange(Bu), 0, I, T=T, G=G)
