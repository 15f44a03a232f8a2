"""``ops.dense_knn_topk`` (row norms + the fused cosine / top-k kernel of csrc/dense_knn.hip) at k = 100 on normal features of 3,706 x 768
(ML-1M's item count with a text-embedding width) and 25,000 x 256, beside a composition of torch's own operators on the same device:
rows normalised once, then per chunk of --chunk rows ``Fn[chunk] @ Fn.T``, the diagonal zeroed, ``torch.topk`` (the composition keeps
zero dots as candidates and holds a chunk x n block in memory: it is the yardstick for time, not for the contract). Device-event times,
--warmup runs first, then the median of --reps runs. Prints one JSON line. Stand-alone: nothing is gated on these figures.

    python tools/time_dense_knn.py [--reps 7] [--warmup 2] [--small]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sibrar_amd as S                                                            # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {'median_ms': round(statistics.median(ms), 3), 'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3), 'reps': reps}


def torch_composition(F, k, chunk):
    Fn = F / F.norm(dim=1, keepdim=True).clamp_min(1e-30)
    n = F.shape[0]
    vals, idxs = [], []
    for r0 in range(0, n, chunk):
        s = Fn[r0:r0 + chunk] @ Fn.t()
        rows = torch.arange(s.shape[0], device=F.device)
        s[rows, rows + r0] = 0.
        v, i = torch.topk(s, min(k, n), dim=1)
        vals.append(v)
        idxs.append(i)
    return torch.cat(vals), torch.cat(idxs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--chunk', type=int, default=4096)
    ap.add_argument('--k', type=int, default=100)
    ap.add_argument('--small', action='store_true', help='500 x 64 only: a functional check of this script')
    args = ap.parse_args()
    shapes = [(500, 64)] if args.small else [(3706, 768), (25000, 256)]
    out = {'k': args.k, 'device': torch.cuda.get_device_name(0), 'shapes': []}
    for n, d in shapes:
        F = torch.randn(n, d, device='cuda', generator=torch.Generator('cuda').manual_seed(n))
        fused = timed(lambda: S.ops.dense_knn_topk(F, args.k), args.warmup, args.reps)
        comp = timed(lambda: torch_composition(F, args.k, args.chunk), args.warmup, args.reps)
        idx, val, _ = S.ops.dense_knn_topk(F, args.k)
        tv, _ = torch_composition(F, args.k, args.chunk)
        out['shapes'].append({'n': n, 'd': d, 'fused': fused, 'torch': comp, 'tflops_fused': round(2e-9 * n * n * d / fused['median_ms'], 2),
                              'max_value_difference': float((val - tv).abs().max())})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
