"""UserKNN / ItemKNN at the c2 shape (100,000 users x 50,000 items, 5,000,000 synthetic interactions, k = 100, cosine): the time of ``fit``'s
kernel (``ops.knn_topk`` over all rows, one launch) and of one 4096-user chunk of score rows (``ops.csr_rows_times_csr``), device-event
times, median of repeated launches after a warm-up. There is no baseline route in this package to compare with: the figures are recorded
(DESIGN.md 4.16), not gated. One JSON line per model.

    python tools/bench_knn.py [--reps 5] [--small]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import sibrar_amd as S

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--small', action='store_true', help='10,000 x 5,000 with 500,000 interactions: a quick check of the script itself')
args = ap.parse_args()
assert torch.cuda.is_available(), 'this benchmark measures the GPU; there is nothing to measure without one'
dev = 'cuda:0'
n_users, n_items, nnz = (10_000, 5_000, 500_000) if args.small else (100_000, 50_000, 5_000_000)
inter = S.datasets.synthetic_interactions(n_users, n_items, nnz, seed=0)


def median_ms(fn, reps):
    fn()                                                              # warm-up: code object, allocator, the transposed CSR
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(min(out)), float(max(out))


for alg in ('uknn', 'iknn'):
    m = S.ALGORITHMS[alg](S.SimilarityFunctionEnum.cosine, k=100).to(dev)
    m.attach(inter)
    fit = median_ms(lambda: S.ops.knn_topk(m._matrix, 'cosine', 100), args.reps)
    m.fit(inter)
    x, y = m._ops()
    users = torch.randperm(n_users, generator=torch.Generator().manual_seed(1))[:4096].to(dev)
    score = median_ms(lambda: S.ops.csr_rows_times_csr(x, users, y), 2 * args.reps)
    print(json.dumps({'bench': 'knn', 'alg': alg, 'n_users': n_users, 'n_items': n_items, 'nnz': int(inter.nnz), 'k': 100, 'sim': 'cosine',
                      'fit_kernel_ms_median_min_max': [round(v, 3) for v in fit], 'score_4096_users_ms_median_min_max': [round(v, 3) for v in score],
                      'mean_list_length': round(float(m.nbr_len.float().mean()), 2), 'reps': args.reps}), flush=True)
