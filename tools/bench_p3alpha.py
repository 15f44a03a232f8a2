"""P3alpha on synthetic 0/1 data at ML-1M's shape (6,040 users x 3,706 items, about 1,000,000 interactions) and at 100,000 x 25,000 with
5,000,000: the time of ``fit``'s kernel (``ops.p3_walk_dense`` over all rows, one launch) and of one 1,024-user chunk of score rows
(``ops.p3_score_rows``, alpha = 1.9), device-event times, median, minimum and maximum of repeated launches after a warm-up. For comparison,
where both dense operands fit in the free device memory, the plain composition of the same matrix: a dense fp32 ``torch`` product
``(D_i^-1 X^T) @ (D_u^-1 X)`` (the product alone; building the dense operands is not timed). The figures are recorded,
not gated. One JSON line per shape.

    python tools/bench_p3alpha.py [--reps 5] [--small]
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
ap.add_argument('--small', action='store_true', help='2,000 x 1,000 with 50,000 interactions only: a quick check of the script itself')
args = ap.parse_args()
assert torch.cuda.is_available(), 'this benchmark measures the GPU; there is nothing to measure without one'
dev = 'cuda:0'
ALPHA, CHUNK = 1.9, 1024


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
    return [round(float(np.median(out)), 3), round(float(min(out)), 3), round(float(max(out)), 3)]


def dense_composition(inter, w, reps):
    """-> (times, max |product - W| / max W) of the dense product, or (None, None) where the operands do not fit"""
    n, m = inter.shape
    need = 4 * (4 * n * m + m * m) + (1 << 30)                   # x, both operands, one transient; the product
    if need > torch.cuda.mem_get_info()[0]:
        return None, None
    x = torch.zeros(n, m, device=dev)
    coo = inter.tocoo()
    x[torch.from_numpy(coo.row).long().to(dev), torch.from_numpy(coo.col).long().to(dev)] = 1.
    du, di = x.sum(1), x.sum(0)
    right = x / du.clamp(min=1)[:, None]                              # D_u^-1 X
    left = (x / di.clamp(min=1)[None, :]).t().contiguous()            # D_i^-1 X^T
    del x
    out = torch.empty(m, m, device=dev)
    times = median_ms(lambda: torch.matmul(left, right, out=out), reps)
    return times, float((out - w).abs().max() / w.max())


shapes = [(2_000, 1_000, 50_000)] if args.small else [(6_040, 3_706, 1_000_000), (100_000, 25_000, 5_000_000)]
for n_users, n_items, nnz in shapes:
    inter = S.datasets.synthetic_interactions(n_users, n_items, nnz, seed=0)
    m = S.P3alpha(ALPHA).to(dev)
    m.attach(inter)
    w = torch.empty(n_items, n_items, device=dev)
    fit = median_ms(lambda: S.ops.p3_walk_dense(m._matrix, out=w), args.reps)
    m.W = w
    users = torch.randperm(n_users, generator=torch.Generator().manual_seed(1))[:CHUNK].to(dev)
    score = median_ms(lambda: S.ops.p3_score_rows(m._matrix, users, w, ALPHA), 2 * args.reps)
    dense, diff = dense_composition(inter, w, args.reps)
    deg = np.diff(inter.indptr).astype(np.float64)
    print(json.dumps({'bench': 'p3alpha', 'n_users': n_users, 'n_items': n_items, 'nnz': int(inter.nnz), 'alpha': ALPHA,
                      'sum_user_degree_squared': float((deg * deg).sum()), 'fit_kernel_ms_median_min_max': fit,
                      f'score_{CHUNK}_users_ms_median_min_max': score, 'dense_torch_product_ms_median_min_max': dense,
                      'dense_product_max_rel_diff': diff, 'reps': args.reps}), flush=True)
    del w, m
    torch.cuda.empty_cache()
