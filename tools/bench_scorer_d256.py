"""HIP-event medians of three full-catalogue scorer routes at D = 256 in ONE process per shape, on the same inputs
(eval/eval.py:216-222 is the work; the sibling of tools/bench_scorer_f32.py for the 256-wide configs):
  * f32s_d256 : ops.score_topk_f32s_d256 (csrc/score_topk_f32s.hip, the one-wave-per-SIMD kernels: fp32-class products, mask + top-k fused)
  * fp32      : the 'fp32' route of evaluate_recommender_algorithm — fp32 GEMM into a [chunk, I] score matrix, sbr_mask_scores_shard,
                sbr_topk_rows — in the evaluation's own user chunks. THE BASELINE of every ratio printed here.
  * fp16_fused: ops.score_topk_f16 on fp16-rounded copies (the one-pass kernel, route 1)
Shapes (item shard of BASELINE configs[4]: 25,000 items of 200,000 at item_offset 75,000, ~50 exclusions per user inside the shard):
  * c5_shard : 100,000 users
  * chunk    : 262,144 users, the evaluator's fused user chunk of the 1M-user configs
Per shape and list length (k = 20: the narrow kernels, k = 100: the wide ones): milliseconds per pass (median of --reps passes after
two warm-up passes, all passes listed), the new route's MFMA fraction of its six-term floor (6 * 2 * U * I * D / 2.5 PFLOP/s dense bf16)
and its ratio to the fp32 route. Prints one JSON line. The three routes are timed alternately, round by round, so that a drift of the
machine meets all of them.

usage: python tools/bench_scorer_d256.py --shape c5_shard|chunk [--reps N] [--ks 20,100]"""
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
PEAK = 2.5e15
D = 256
I_TOTAL, OFF, I_SHARD, PER = 200_000, 75_000, 25_000, 50
SHAPES = {'c5_shard': 100_000, 'chunk': 262_144}


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _excl(U, seed):
    """PER random exclusions per user inside the shard's item range (global item positions)"""
    rng = np.random.default_rng(seed)
    m = sp.csr_matrix((np.ones(U * PER, dtype=np.int8), (np.repeat(np.arange(U), PER), OFF + rng.integers(0, I_SHARD, size=U * PER))),
                      shape=(U, I_TOTAL))
    m.sum_duplicates()
    m.sort_indices()
    return S.evaluation._csr_to_device(m, DEV)


def run_shape(U, ks, reps):
    ops = S.ops
    g = torch.Generator().manual_seed(U + D)
    u32 = (torch.randn(U, D, generator=g) / 8).to(DEV)
    i32 = (torch.randn(I_SHARD, D, generator=g) / 8).to(DEV)
    users = torch.arange(U, device=DEV)
    ex = _excl(U, 1)
    planes = ops.split_bf16x3(i32)
    u16, i16 = ops.cast_f16(u32), ops.cast_f16(i32)
    bs = max(256, min(16384, max(1, (1 << 31) // I_SHARD)))      # evaluate_recommender_algorithm's fp32 chunk
    floor_ms = 6 * 2 * U * I_SHARD * D / PEAK * 1e3
    res = {'U': U, 'I': I_SHARD, 'D': D, 'item_offset': OFF, 'excl_per_user': PER, 'fp32_user_chunk': bs,
           'six_term_floor_ms': round(floor_ms, 4)}
    for k in ks:
        h32, h16 = ops.ScorerExclusions(), ops.ScorerExclusions()

        def f32s_d256():
            return ops.score_topk_f32s_d256(u32, planes, k, users, ex[0], ex[1], item_offset=OFF, exclusions=h32)

        def fp32_route():
            out = []
            for s in range(0, U, bs):
                sc = ops.ScoreAllFn.apply(u32[s:s + bs], i32)
                ops.mask_scores_(sc, users[s:s + bs], ex[0], ex[1], item_offset=OFF)
                v, i = ops.topk_rows(sc, k)
                out.append(i + OFF)
            return out

        def fp16_fused():
            return ops.score_topk_f16(u16, i16, k, users, ex[0], ex[1], item_offset=OFF, exclusions=h16)

        routes = {'f32s_d256': f32s_d256, 'fp32': fp32_route, 'fp16_fused': fp16_fused}
        prev = ops.score_topk_route(1)
        try:
            for _ in range(2):
                for f in routes.values():
                    f()
            torch.cuda.synchronize()
            times = {name: [] for name in routes}
            for _ in range(reps):
                for name, f in routes.items():
                    times[name].append(_timed(f))
            fi = f32s_d256()[1]
            ri = torch.cat(fp32_route())
        finally:
            ops.score_topk_route(prev)
        r = {}
        for name, t in times.items():
            r[name + '_ms'] = round(float(np.median(t)), 4)
            r[name + '_all_ms'] = [round(x, 4) for x in t]
        r['f32s_d256_mfma_fraction_of_six_term_floor'] = round(floor_ms / r['f32s_d256_ms'], 4)
        r['fp32_ms_over_f32s_d256_ms'] = round(r['fp32_ms'] / r['f32s_d256_ms'], 3)
        r['f32s_d256_ms_over_fp16_fused_ms'] = round(r['f32s_d256_ms'] / r['fp16_fused_ms'], 3)
        r['f32s_d256_positions_equal_fp32'] = round(float((ri == fi).float().mean()), 6)
        res[f'k{k}'] = r
        del fi, ri
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', required=True, choices=sorted(SHAPES))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--ks', default='20,100')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_scorer_d256 needs the GPU: a CPU run says nothing about these times'
    out = {'tool': 'bench_scorer_d256', 'device': torch.cuda.get_device_name(0), 'shape': a.shape, 'baseline': 'fp32 route, same process'}
    out.update(run_shape(SHAPES[a.shape], [int(k) for k in a.ks.split(',')], a.reps))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
