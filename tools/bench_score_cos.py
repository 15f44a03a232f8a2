"""DeepMF's cosine scorer: ``ops.ScoreCosFn`` (one kernel each way) against the composition available without it —
``L2NormalizeFn`` (eps 1e-8) on both operands -> ``ScoreDotFn`` -> ``clamp(min=mu)`` and the mirror image in the backward —, forward +
backward, device-event times over alternating repetitions; the bytes the algorithm needs ((B D + B N D) * 4 read, B N * 4 written, and
the same again plus the gradients in the backward) over the measured time, next to the bytes each variant's kernels move (counted
from their loads and stores); then the DeepMF training step on the ML-1M-shaped world
(5,816 x 3,299, towers [., 128, 64]) through the Trainer at batch 256 and 4096. One JSON line per measurement.

    python tools/bench_score_cos.py [--reps 200] [--no-step]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import sibrar_amd as S
import bench

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=200)
ap.add_argument('--no-step', action='store_true')
args = ap.parse_args()
assert torch.cuda.is_available(), 'this benchmark measures the GPU; there is nothing to measure without one'
dev, mu = 'cuda:0', 1e-6
ops = S.ops


def fused(u, i, g):
    out = ops.ScoreCosFn.apply(u, i, mu)
    out.backward(g)


def composed(u, i, g):
    B, N, D = i.shape
    un = ops.L2NormalizeFn.apply(u, 1e-8)
    inn = ops.L2NormalizeFn.apply(i.reshape(B * N, D), 1e-8).reshape(B, N, D)
    out = ops.ScoreDotFn.apply(un, inn).clamp(min=mu)
    out.backward(g)


def moved_fused(B, N, D):
    """bytes the two kernels of ScoreCosFn read and write (counted from their loads and stores)"""
    rows, ent = (B + B * N) * D * 4, B * N * 4
    saved = ent + (B + B * N) * 8                                     # un-floored cosine + two inverse norms per row
    fwd = rows + ent + saved                                          # read u, i; write scores and the saved statistics
    bwd = rows + ent + saved + rows                                   # read u, i, g and the statistics; write dU, dI
    return fwd + bwd


def moved_composed(B, N, D):
    """the same count for L2NormalizeFn x 2 -> ScoreDotFn -> clamp and their backward kernels"""
    rows, ent, inv = (B + B * N) * D * 4, B * N * 4, (B + B * N) * 4
    norm_fwd = 2 * rows + rows + inv                                  # rows read twice (norm, then scale), normalised copy + 1 / norm written
    dot_fwd = rows + ent                                              # normalised copies read, scores written
    clamp_fwd = 2 * ent
    clamp_bwd = 3 * ent                                               # grad and input read, grad written
    dot_bwd = ent + rows + rows                                       # g and the normalised copies read, their gradients written
    norm_bwd = (2 * rows + inv) + rows + rows                         # dy and y read for the dot, read again for dx (cache permitting), dx written
    return norm_fwd + dot_fwd + clamp_fwd + clamp_bwd + dot_bwd + norm_bwd


def timed(fn, u, i, g, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        u.grad = i.grad = None
        fn(u, i, g)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


for B in (256, 8192):
    for D in (64, 128):
        N = 4
        gen = torch.Generator().manual_seed(B + D)
        u = torch.randn(B, D, generator=gen).to(dev).requires_grad_(True)
        i = torch.randn(B, N, D, generator=gen).to(dev).requires_grad_(True)
        g = torch.randn(B, N, generator=gen).to(dev)
        for fn in (fused, composed):
            timed(fn, u, i, g, 20)                                    # warm-up: code objects, allocator
        ms = {'fused': [], 'composed': []}
        for _ in range(5):                                            # alternating blocks: drift hits both alike
            ms['fused'].append(timed(fused, u, i, g, args.reps))
            ms['composed'].append(timed(composed, u, i, g, args.reps))
        # algorithmic bytes: forward reads u and i, writes the scores; backward reads g, u, i and writes dU, dI
        fwd = (B * D + B * N * D) * 4 + B * N * 4
        bwd = B * N * 4 + 2 * (B * D + B * N * D) * 4
        row = {'bench': 'score_cos_fwd_bwd', 'B': B, 'N': N, 'D': D, 'algorithmic_bytes': fwd + bwd,
               'fused_bytes_moved': moved_fused(B, N, D), 'composed_bytes_moved': moved_composed(B, N, D)}
        for k, v in ms.items():
            med = float(np.median(v))
            row[f'{k}_ms'] = round(med, 5)
            row[f'{k}_ms_spread'] = [round(min(v), 5), round(max(v), 5)]
            row[f'{k}_algorithmic_GBps'] = round((fwd + bwd) / med / 1e6, 1)
            row[f'{k}_moved_over_algorithmic'] = round(row[f'{k}_bytes_moved'] / (fwd + bwd), 2)
        row['note'] = 'host-launched autograd round trip: at these sizes launch overhead is part of every figure'
        print(json.dumps(row), flush=True)

if not args.no_step:
    ds = S.SyntheticDataset(5816, 3299, 651034, seed=0, n_negative_samples=10, holdout_per_user=2, item_popularity=1.0)
    torch.manual_seed(42)
    net = S.ALGORITHMS['dmf'].build_from_conf(dict(u_mid_layers=[128], i_mid_layers=[128], final_dimension=64), ds)
    loss = S.RecBinaryCrossEntropy(n_items=ds.n_items, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=10)
    tr = S.Trainer(net, None, None, loss, {'learn': {'lr': 1e-3, 'wd': 1e-6, 'optimizer': 'adamw'}, 'run_settings': {'device': dev}})
    net.train()
    for B in (256, 4096):
        ld = S.NegativeSamplingDataLoader(ds, batch_size=B, shuffle=True, device=dev, prefetch=4)
        it = bench.epochs(ld)
        for _ in range(15):
            tr.train_step(*next(it))
        torch.cuda.synchronize()
        n = 60
        t0 = time.perf_counter()
        for _ in range(n):
            out = tr.train_step(*next(it))
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n
        ld.close()
        print(json.dumps({'bench': 'deepmf_train_step', 'B': B, 'neg': 10, 'towers': '[., 128, 64]', 'ms_per_step': round(dt * 1e3, 4),
                          'k_interactions_per_s': round(B / dt / 1e3, 1), 'loss': round(float(out[0]), 5)}), flush=True)
