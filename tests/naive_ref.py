"""numpy restatements for PopularItems / RandomItems (csrc/shared_rank.hip): what sbr_shared_rank_topk and sbr_uniform_rows_f32 must give,
written the slow and obvious way. A plain module: no fixtures, no pytest hooks.

``shared_rank_topk_ref`` does not walk a ranking: it masks the user's excluded positions out of the score vector, sorts what is left
stably on (-score, index) and pads — the definition the walk is a shortcut for. ``philox4x32_10`` is Philox4x32-10 (Salmon, Moraes,
Dror, Shaw, SC 2011) in uint64 arithmetic; ``uniform_rows_ref`` applies the counter layout and the [0, 1) mapping of include/sibrar_hip.h.
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
LOW = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)

# Random123's first known-answer vector for philox4x32-10 (zero counter, zero key), and three answers of rocRAND's host-callable engine
# (rocrand/rocrand_philox4x32_10.h: philox4x32_10_engine(seed, subsequence, offset), whose counter is (offset / 4 low, offset / 4 high,
# subsequence low, subsequence high) and whose key is the two halves of seed), taken with a small host program: ((key0, key1), counter,
# output block). The zero vector and the engine agree.
KNOWN_ANSWERS = (
    ((0x00000000, 0x00000000), (0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    # seed 3, user 7, block 2
    ((0x00000003, 0x00000000), (0x00000007, 0x00000000, 0x00000002, 0x00000000), (0x57011000, 0x57d2963f, 0x36735324, 0x022455e5)),
    # seed 0x123456789abcdef0, user 2^31 + 5, block 249
    ((0x9abcdef0, 0x12345678), (0x80000005, 0x00000000, 0x000000f9, 0x00000000), (0xe1cf811a, 0x96d98aed, 0x5faa87bc, 0x6463b322)),
    # seed 2^64 - 1, user 2^40 + 3, block 0
    ((0xffffffff, 0xffffffff), (0x00000003, 0x00000100, 0x00000000, 0x00000000), (0xad53eff0, 0x3e667db9, 0x4b2522b5, 0xe8d35a5d)),
)


def philox4x32_10(counter, key):
    """counter: uint32 [..., 4], key: (k0, k1) -> uint32 [..., 4], every step in uint64 so that nothing wraps unseen"""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                                # < 2^64: both factors are below 2^32
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & LOW, (p0 >> S32) ^ c[3] ^ k1, p0 & LOW]
        k0, k1 = (k0 + W0) & LOW, (k1 + W1) & LOW
    return np.stack(c, axis=-1).astype(np.uint32)


def unit_float(x):
    """the top 24 bits of a word times 2^-24: float32 in [0, 1), exact"""
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def uniform_rows_ref(seed, u_idx, n_items):
    """float32 [len(u_idx), n_items]: U(seed, user id, j) with key = the halves of seed, counter = (id low, id high, j / 4, 0), word j % 4"""
    seed = int(seed)
    u = np.asarray(u_idx, dtype=np.int64).astype(np.uint64)
    nb = (n_items + 3) // 4
    ctr = np.zeros((len(u), nb, 4), dtype=np.uint32)
    ctr[:, :, 0] = (u & LOW).astype(np.uint32)[:, None]
    ctr[:, :, 1] = (u >> S32).astype(np.uint32)[:, None]
    ctr[:, :, 2] = np.arange(nb, dtype=np.uint32)[None, :]
    words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    return unit_float(words.reshape(len(u), nb * 4)[:, :n_items])


def stable_order(score):
    """positions by (score descending, index ascending); the two zeros are one score"""
    s = np.asarray(score, dtype=np.float32) + np.float32(0)          # -0.0 + 0.0 = +0.0
    return np.lexsort((np.arange(len(s)), -s.astype(np.float64))).astype(np.int32)


def shared_rank_topk_ref(score, u_idx, indptr, indices, k):
    """-> (val float32 [Bu, k], idx int32 [Bu, k]): mask, stable sort on (-score, index), pad with (-inf, -1). ``score`` may hold -inf
    (a real entry: it keeps its index) but no NaN."""
    score = np.asarray(score, dtype=np.float32)
    n = len(score)
    val = np.full((len(u_idx), k), -np.inf, dtype=np.float32)
    idx = np.full((len(u_idx), k), -1, dtype=np.int32)
    for b, u in enumerate(np.asarray(u_idx, dtype=np.int64)):
        allowed = np.ones(n, dtype=bool)
        allowed[np.asarray(indices[indptr[u]:indptr[u + 1]], dtype=np.int64)] = False
        pos = np.flatnonzero(allowed)
        key = -(score[pos] + np.float32(0)).astype(np.float64)
        pos = pos[np.lexsort((pos, key))][:k]
        val[b, :len(pos)], idx[b, :len(pos)] = score[pos], pos
    return val, idx


def brute_force_topk(score, excluded, k):
    """one user, the slowest way: pick the best remaining position k times"""
    score = np.asarray(score, dtype=np.float32)
    left = [p for p in range(len(score)) if p not in set(int(e) for e in excluded)]
    out = []
    while left and len(out) < k:
        best = left[0]
        for p in left[1:]:
            if score[p] > score[best]:                               # strictly better only: the lowest position wins a tie, -0.0 == +0.0
                best = p
        out.append(best)
        left.remove(best)
    return out


def load_g27():
    with open(os.path.join(GOLDEN, 'g27_naive.json')) as fh:
        meta = json.load(fh)
    with np.load(os.path.join(GOLDEN, 'g27_naive.npz')) as f:
        return {k: f[k] for k in f.files}, meta
