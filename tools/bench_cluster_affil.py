"""ECF's cluster affiliation: ``ops.ClusterAffilFn`` (cosine form: normalisations, logits, clamp, exact top-k mask, softmax mask with the
straight-through gradient and sigmoid in one op each way) against the composition available without it — torch ``F.normalize`` ->
``linear_nt`` / ``matmul_nn`` / ``matmul_tn`` -> torch ``clamp``, ``topk`` + scatter, ``softmax``, ``sigmoid`` and autograd's mirror image
of those —, one training step's forward + backward over the whole catalogue at (I, D, C, top) = (45056, 100, 64, 20) and
(32768, 128, 256, 20): device-event times over alternating repetitions. The composition is the baseline, not the code under test; its
top-k breaks ties as torch does. One JSON line per shape.

    python tools/bench_cluster_affil.py [--reps 100]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import sibrar_amd as S
from torch.nn import functional as F

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=100)
args = ap.parse_args()
assert torch.cuda.is_available(), 'this benchmark measures the GPU; there is nothing to measure without one'
dev = 'cuda:0'
ops = S.ops
TEMP = 2.0


def fused(table, clusters, top, g_x, g_t):
    t, x = ops.ClusterAffilFn.apply(table, clusters, None, top, TEMP)
    torch.autograd.backward([x, t], [g_x, g_t])


class _LinearNT(torch.autograd.Function):
    """x @ w^T through the library's GEMMs, both gradients"""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return ops.linear_nt(x, w)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        return ops.matmul_nn(g, w), ops.matmul_tn(g, x)


def composed(table, clusters, top, g_x, g_t):
    t = torch.clamp(_LinearNT.apply(F.normalize(table), F.normalize(clusters)), min=-1., max=1.)
    m = torch.zeros_like(t).scatter_(-1, t.detach().topk(top).indices, 1.)
    p = torch.softmax(t / TEMP, dim=-1)
    x = torch.sigmoid(t) * (p + (m - p).detach())
    torch.autograd.backward([x, t], [g_x, g_t])


def timed(fn, table, clusters, top, g_x, g_t, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        table.grad = clusters.grad = None
        fn(table, clusters, top, g_x, g_t)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


for R, D, C, top in ((45056, 100, 64, 20), (32768, 128, 256, 20)):
    gen = torch.Generator().manual_seed(R + D + C)
    table = torch.randn(R, D, generator=gen).to(dev).requires_grad_(True)
    clusters = torch.randn(C, D, generator=gen).to(dev).requires_grad_(True)
    g_x, g_t = (torch.randn(R, C, generator=gen) / R).to(dev), (torch.randn(R, C, generator=gen) / R).to(dev)
    grads = {}
    for name, fn in (('fused', fused), ('composed', composed)):
        timed(fn, table, clusters, top, g_x, g_t, 10)                 # warm-up: code objects, allocator
        grads[name] = (table.grad.clone(), clusters.grad.clone())
    # the two variants compute the same gradients (fp32 reorderings and rows with a near-tie at the mask boundary apart)
    agree = [float((a - b).norm() / b.norm()) for a, b in zip(grads['fused'], grads['composed'])]
    ms = {'fused': [], 'composed': []}
    for _ in range(5):                                                # alternating blocks: drift hits both alike
        ms['fused'].append(timed(fused, table, clusters, top, g_x, g_t, args.reps))
        ms['composed'].append(timed(composed, table, clusters, top, g_x, g_t, args.reps))
    row = {'bench': 'cluster_affil_fwd_bwd', 'R': R, 'D': D, 'C': C, 'top': top, 'logits_bytes': R * C * 4, 'table_bytes': R * D * 4,
           'rel_diff_table_grad': agree[0], 'rel_diff_cluster_grad': agree[1]}
    for k, v in ms.items():
        row[f'{k}_ms'] = round(float(np.median(v)), 5)
        row[f'{k}_ms_spread'] = [round(min(v), 5), round(max(v), 5)]
    row['fused_over_composed'] = round(row['fused_ms'] / row['composed_ms'], 3)
    row['note'] = 'host-launched autograd round trip, cosine form with an upstream gradient into t'
    print(json.dumps(row), flush=True)
