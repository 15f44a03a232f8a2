"""The simplified ProtoMF family's training logit: ``ops.ProtoScoreFn`` (lookup, normalisations, cosine, clamp, weight gather, ReLU and the
dot over the prototypes in one op each way) against the composed route of the same commit — ``ops.ProtoCosFn`` -> ``ops.LookupFn`` ->
torch ``relu`` -> ``ops.ScoreDotFn`` and autograd's mirror image of those —, one training step's forward + backward of a UProtoMFs-shaped
side at (B, N + 1, D, P) = (8192, 4, 100, 20) and (256, 4, 100, 20): device-event times over alternating blocks of repetitions. The
composed route is the baseline, not the code under test. One JSON line per shape.

    python tools/bench_proto_score.py [--reps 100]
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
ap.add_argument('--reps', type=int, default=100)
args = ap.parse_args()
assert torch.cuda.is_available(), 'this benchmark measures the GPU; there is nothing to measure without one'
dev = 'cuda:0'
ops = S.ops


def fused(table, u, protos, weights, i, g):
    ops.ProtoScoreFn.apply(table, u, protos, weights, i.reshape(-1), i.shape[1]).backward(g)


def composed(table, u, protos, weights, i, g):
    ops.ScoreDotFn.apply(ops.ProtoCosFn.apply(table, u, protos), torch.relu(ops.LookupFn.apply(weights, i))).backward(g)


def timed(fn, params, rest, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        for p in params:
            p.grad = None
        fn(params[0], rest[0], params[1], params[2], rest[1], rest[2])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


for B, N1, D, P, n_users, n_items in ((8192, 4, 100, 20, 60000, 40000), (256, 4, 100, 20, 60000, 40000)):
    gen = torch.Generator().manual_seed(B + D + P)
    params = [(torch.randn(n_users, D, generator=gen) * 0.5).to(dev).requires_grad_(True),
              torch.randn(P, D, generator=gen).to(dev).requires_grad_(True),
              (torch.randn(n_items, P, generator=gen) * 0.5).to(dev).requires_grad_(True)]
    rest = [torch.randint(0, n_users, (B,), generator=gen).to(dev), torch.randint(0, n_items, (B, N1), generator=gen).to(dev),
            (torch.randn(B, N1, generator=gen) / B).to(dev)]
    for fn in (fused, composed):
        timed(fn, params, rest, 10)                                   # warm-up: code objects, allocator
    ms = {'fused': [], 'composed': []}
    for _ in range(5):                                                # alternating blocks: drift hits both alike
        ms['fused'].append(timed(fused, params, rest, args.reps))
        ms['composed'].append(timed(composed, params, rest, args.reps))
    row = {'bench': 'proto_score_fwd_bwd', 'B': B, 'N+1': N1, 'D': D, 'P': P}
    for k, v in ms.items():
        row[f'{k}_ms'] = round(float(np.median(v)), 5)
        row[f'{k}_ms_spread'] = [round(min(v), 5), round(max(v), 5)]
    row['fused_over_composed'] = round(row['fused_ms'] / row['composed_ms'], 3)
    row['note'] = 'host-launched autograd round trip, all three dense table gradients (zero fill + scatter) included in both'
    print(json.dumps(row), flush=True)
