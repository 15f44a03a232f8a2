"""HIP-event medians of the three full-catalogue scorer routes at several list lengths in ONE process, alternating (a sibling of
tools/bench_scorer_f32.py for the wide lists, k = 33 .. 128):
  * fp32      : the 'fp32' route of evaluate_recommender_algorithm (fp32 GEMM into a [chunk, I] score matrix, sbr_mask_scores,
                sbr_topk_rows) in the evaluation's own user chunks — what a list longer than 32 gets without ``fused_max_k``
  * fp16_fused: ops.score_topk_f16 on fp16-rounded copies (one-pass kernel)
  * fp32_fused: ops.score_topk_f32s (D = 64, 128 only)
Shapes: c2 (100k x 50k x 128, 50 random exclusions per user) and the c5 shard (100k x 25k x 256). Every (route, k) variant is timed
``--reps`` times per alternation, the variants take turns ``--alternations`` times; per variant the median of each alternation and their
spread are reported. With ``--stats`` the fused routes' final fill counts are read back from the workspace at each k: entries per user
that enter the final selection (all of them lie at or above the user's last threshold). Prints one JSON line.

usage: python tools/bench_scorer_wide.py [--k 20,100] [--reps 7] [--alternations 3] [--only c2,c5_shard] [--routes fp32,fp16_fused,fp32_fused] [--stats]"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sibrar_amd as S  # noqa: E402

DEV = 'cuda'
SHAPES = {'c2': (100_000, 50_000, 128, 50), 'c5_shard': (100_000, 25_000, 256, 50)}


def _times_ms(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def _excl(U, I, per, seed):
    rng = np.random.default_rng(seed)
    m = sp.csr_matrix((np.ones(U * per, dtype=np.int8), (np.repeat(np.arange(U), per), rng.integers(0, I, size=U * per))), shape=(U, I))
    m.sum_duplicates()
    m.sort_indices()
    return S.evaluation._csr_to_device(m, DEV)


def _fill_stats(entry, maxw, u_op, i_op, I, k, users, ex):
    """one call of a fused C entry with a workspace of our own -> entries per user left in the candidate buffers (users of full waves)"""
    from importlib import import_module
    _lib = import_module(S.ops.__name__.rsplit('.', 1)[0] + '._lib')
    Bu, D = u_op.shape
    nnz = int(ex[1].numel())
    ws = torch.zeros(int(getattr(_lib.lib(), entry + '_workspace')(Bu, I, k)), device=DEV, dtype=torch.uint8)
    ev = torch.empty(int(_lib.lib().sbr_score_topk_f16_events_bytes(Bu, nnz)) + 16, device=DEV, dtype=torch.uint8)
    val = torch.empty(Bu, k, device=DEV)
    idx = torch.empty(Bu, k, device=DEV, dtype=torch.int32)
    _lib.call(entry, u_op.data_ptr(), i_op.data_ptr(), D, Bu, I, users.data_ptr(), ex[0].data_ptr(), ex[1].data_ptr(), nnz, 0, k,
              val.data_ptr(), idx.data_ptr(), ws.data_ptr(), ws.numel(), ev.data_ptr(), ev.numel(), 1, _lib.stream())
    torch.cuda.synchronize()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    padded = -(-Bu // 32) * 32 + 32 * maxw + 32 * n_cu
    cnt = ws[padded * 2 * 256 * 8:].view(torch.int32)[:padded * 4].view(padded, 4)[:Bu]        # (n0, threshold bits, n1, threshold bits)
    full = (Bu // 32 // n_cu) * n_cu * 32 if (Bu // 32) % n_cu else Bu                          # rows of remainder units hold no entries
    n = (cnt[:full, 0] + cnt[:full, 2]).float()
    return {'users': int(full), 'entries_mean': round(float(n.mean()), 1), 'entries_p50': float(n.median()), 'entries_max': float(n.max()),
            'share_over_128': round(float((n > 128).float().mean()), 4), 'share_over_256': round(float((n > 256).float().mean()), 4)}


def run_shape(U, I, D, per, ks, routes, reps, alternations, stats):
    ops = S.ops
    g = torch.Generator().manual_seed(U + I + D)
    u32 = (torch.randn(U, D, generator=g) / 8).to(DEV)
    i32 = (torch.randn(I, D, generator=g) / 8).to(DEV)
    users = torch.arange(U, device=DEV)
    ex = _excl(U, I, per, 1)
    bs = max(256, min(16384, max(1, (1 << 31) // I)))
    variants = {}
    if 'fp32' in routes:
        def fp32_route(k):
            for s in range(0, U, bs):
                sc = ops.ScoreAllFn.apply(u32[s:s + bs], i32)
                ops.mask_scores_(sc, users[s:s + bs], ex[0], ex[1])
                ops.topk_rows(sc, k)
        for k in ks:
            variants[f'fp32 k={k}'] = (lambda k=k: fp32_route(k))
    u16 = i16 = planes = None
    if 'fp16_fused' in routes:
        u16, i16 = ops.cast_f16(u32), ops.cast_f16(i32)
        h16 = ops.ScorerExclusions()
        for k in ks:
            variants[f'fp16_fused k={k}'] = (lambda k=k: ops.score_topk_f16(u16, i16, k, users, ex[0], ex[1], exclusions=h16))
    if 'fp32_fused' in routes and D in (64, 128):
        planes = ops.split_bf16x3(i32)
        h32 = ops.ScorerExclusions()
        for k in ks:
            variants[f'fp32_fused k={k}'] = (lambda k=k: ops.score_topk_f32s(u32, planes, k, users, ex[0], ex[1], exclusions=h32))
    res = {'U': U, 'I': I, 'D': D, 'excl_per_user': per, 'reps': reps, 'alternations': alternations, 'variants': {}}
    for fn in variants.values():                             # warm-up: allocator, event streams, code objects
        fn()
    torch.cuda.synchronize()
    medians = {name: [] for name in variants}
    for _ in range(alternations):
        for name, fn in variants.items():
            medians[name].append(round(float(np.median(_times_ms(fn, reps))), 4))
    for name, m in medians.items():
        res['variants'][name] = {'median_ms': round(float(np.median(m)), 4), 'per_alternation_ms': m, 'spread_ms': round(max(m) - min(m), 4)}
    if stats:
        res['buffers'] = {}
        for k in ks:
            if u16 is not None:
                res['buffers'][f'fp16_fused k={k}'] = _fill_stats('sbr_score_topk_f16', 15, u16, i16, I, k, users, ex)
            if planes is not None:
                res['buffers'][f'fp32_fused k={k}'] = _fill_stats('sbr_score_topk_f32s', 7, u32, planes, I, k, users, ex)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--k', default='20,100')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--alternations', type=int, default=3)
    ap.add_argument('--only', default='c2,c5_shard')
    ap.add_argument('--routes', default='fp32,fp16_fused,fp32_fused')
    ap.add_argument('--stats', action='store_true')
    a = ap.parse_args()
    ks = [int(k) for k in a.k.split(',')]
    out = {'tool': 'bench_scorer_wide', 'device': torch.cuda.get_device_name(0), 'k': ks}
    for name in a.only.split(','):
        U, I, D, per = SHAPES[name]
        out[name] = run_shape(U, I, D, per, ks, a.routes.split(','), a.reps, a.alternations, a.stats)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
