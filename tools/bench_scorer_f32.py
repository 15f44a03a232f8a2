"""HIP-event medians of three full-catalogue scorer routes in ONE process, on the same inputs (eval/eval.py:216-222 is the work):
  * f32s      : ops.score_topk_f32s (csrc/score_topk_f32s.hip: fp32-class products on the bf16 pipe, mask + top-k fused)
  * fp32      : the 'fp32' route of evaluate_recommender_algorithm — fp32 GEMM into a [chunk, I] score matrix, sbr_mask_scores,
                sbr_topk_rows — in the evaluation's own user chunks
  * fp16_fused: ops.score_topk_f16 on fp16-rounded copies (the one-pass kernel, route 1)
Shapes: c2 (100k x 50k x 128, 50 random exclusions per user, top-20), c1 (ML-1M: 5,816 x 3,299 x 64, top-20), and the c5 shard
(100k x 25k x 256) only if the f32s route takes D = 256. Per shape: milliseconds per pass, the f32s route's fraction of its six-term
roofline (6 * 2 * U * I * D / 2.5 PFLOP/s) and the one-time split cost of the item matrix. Prints one JSON line.

usage: python tools/bench_scorer_f32.py [--reps N] [--only c2,c1]"""
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
SHAPES = {'c2': (100_000, 50_000, 128, 20, 50), 'c1': (5_816, 3_299, 64, 20, 165), 'c5_shard': (100_000, 25_000, 256, 20, 50)}


def _median_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), [round(x, 4) for x in out]


def _excl(U, I, per, seed):
    rng = np.random.default_rng(seed)
    m = sp.csr_matrix((np.ones(U * per, dtype=np.int8), (np.repeat(np.arange(U), per), rng.integers(0, I, size=U * per))), shape=(U, I))
    m.sum_duplicates()
    m.sort_indices()
    return S.evaluation._csr_to_device(m, DEV)


def run_shape(U, I, D, k, per, reps):
    ops = S.ops
    g = torch.Generator().manual_seed(U + I + D)
    u32 = (torch.randn(U, D, generator=g) / 8).to(DEV)
    i32 = (torch.randn(I, D, generator=g) / 8).to(DEV)
    users = torch.arange(U, device=DEV)
    ex = _excl(U, I, per, 1)
    res = {'U': U, 'I': I, 'D': D, 'k': k, 'excl_per_user': per}
    split_ms, _ = _median_ms(lambda: ops.split_bf16x3(i32), reps)
    res['split_ms'] = round(split_ms, 4)
    planes = ops.split_bf16x3(i32)
    fi = None
    if ops.score_topk_f32s_supported(D, k):
        holder = ops.ScorerExclusions()
        f = lambda: ops.score_topk_f32s(u32, planes, k, users, ex[0], ex[1], exclusions=holder)
        ms, all_ms = _median_ms(f, reps)
        res['f32s_ms'], res['f32s_all_ms'] = round(ms, 4), all_ms
        res['f32s_six_term_floor_ms'] = round(6 * 2 * U * I * D / PEAK * 1e3, 4)
        res['f32s_roofline_fraction'] = round(res['f32s_six_term_floor_ms'] / ms, 4)
        fi = f()[1]
    # the 'fp32' route in evaluate_recommender_algorithm's chunks (<= 8 GiB of scores per chunk)
    bs = max(256, min(16384, max(1, (1 << 31) // I)))

    def fp32_route():
        out = []
        for s in range(0, U, bs):
            sc = ops.ScoreAllFn.apply(u32[s:s + bs], i32)
            ops.mask_scores_(sc, users[s:s + bs], ex[0], ex[1])
            out.append(ops.topk_rows(sc, k))
        return out
    ms, all_ms = _median_ms(fp32_route, max(3, reps // 3), warm=1)
    res['fp32_ms'], res['fp32_all_ms'] = round(ms, 4), all_ms
    if fi is not None:
        ri = torch.cat([o[1] for o in fp32_route()])
        res['f32s_positions_equal_fp32'] = round(float((ri == fi).float().mean()), 6)
        res['f32s_speedup_over_fp32'] = round(res['fp32_ms'] / res['f32s_ms'], 3)
    u16, i16 = ops.cast_f16(u32), ops.cast_f16(i32)
    prev = ops.score_topk_route(1)
    try:
        holder16 = ops.ScorerExclusions()
        ms, all_ms = _median_ms(lambda: ops.score_topk_f16(u16, i16, k, users, ex[0], ex[1], exclusions=holder16), reps)
    finally:
        ops.score_topk_route(prev)
    res['fp16_fused_ms'], res['fp16_fused_all_ms'] = round(ms, 4), all_ms
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--only', default='c2,c1,c5_shard')
    a = ap.parse_args()
    out = {'tool': 'bench_scorer_f32', 'device': torch.cuda.get_device_name(0)}
    for name in a.only.split(','):
        U, I, D, k, per = SHAPES[name]
        if not S.ops.score_topk_f32s_supported(D, k):
            out[name] = {'skipped': f'D = {D} is not supported by the f32s route'}
            continue
        out[name] = run_shape(U, I, D, k, per, a.reps)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
