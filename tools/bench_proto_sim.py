"""ProtoMF's prototype side: ``ops.ProtoSimFn`` (lookup, normalisations, similarity, clamp and both arg-min regularisers in one op each
way) against the composition available without it — ``LookupFn`` -> ``L2NormalizeFn`` on rows and prototypes -> ``linear_nt`` -> torch
``1 + x``, ``clamp`` and the two ``min`` reductions, and autograd's mirror image of those in the backward —, one training step's forward
+ backward at (R, D, P) = (45056, 100, 20) and (32768, 128, 64): device-event times over alternating repetitions, and the bytes each
variant's kernels move (counted from their loads and stores) against the algorithmic R D 4 per direction. The composition is the
baseline, not the code under test. One JSON line per shape.

    python tools/bench_proto_sim.py [--reps 100]
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
W_PROTO, W_BATCH = 1.0, 1.0


def fused(table, idx, protos, g):
    sim, proto_loss, batch_loss = ops.ProtoSimFn.apply(table, idx, protos)
    torch.autograd.backward([sim, W_PROTO * proto_loss + W_BATCH * batch_loss], [g, None])


class _Linear(torch.autograd.Function):
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


def composed(table, idx, protos, g):
    e = ops.LookupFn.apply(table, idx)
    sim = torch.clamp(1 + _Linear.apply(ops.L2NormalizeFn.apply(e), ops.L2NormalizeFn.apply(protos)), min=0., max=2.)
    dis = 2 - sim
    reg = W_PROTO * dis.min(dim=0).values.mean() + W_BATCH * dis.min(dim=1).values.mean()
    torch.autograd.backward([sim, reg], [g, None])


def moved_fused(R, D, P):
    """bytes of ProtoSimFn's kernels: forward reads the rows once, writes sim, the un-clamped cosine and the per-row statistics; backward
    reads the rows twice (once for dE's projection term, once for dP), G and the cosine once per output tile column, writes dE and the dP
    partials; the scatter into the table gradient reads dE and writes the touched rows"""
    rows, ent = R * D * 4, R * P * 4
    fwd = rows + 2 * ent + R * 12
    d_tiles = -(-D // 64)
    bwd = 2 * rows + rows + (1 + d_tiles) * 2 * ent + 2 * R * 12
    scatter = 2 * rows
    return fwd + bwd + scatter


def moved_composed(R, D, P):
    rows, ent = R * D * 4, R * P * 4
    lookup = 2 * rows                                                 # gather: read, write the copy
    norm = 3 * rows                                                   # read twice (norm, scale), write the normalised copy
    gemm = rows + ent
    elementwise_fwd = 2 * ent * 3 + 2 * ent                           # 1 + x, clamp, 2 - x (read + write each), two min reductions (read)
    elementwise_bwd = 2 * ent * 4                                     # min scatters, 2 - x, clamp mask, accumulation of the three gradients
    gemm_bwd = (ent + rows) + (ent + rows)                            # dX = G W (write rows), dW = G^T X (read rows)
    norm_bwd = 4 * rows
    scatter = 2 * rows
    return lookup + norm + gemm + elementwise_fwd + elementwise_bwd + gemm_bwd + norm_bwd + scatter


def timed(fn, table, idx, protos, g, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        table.grad = protos.grad = None
        fn(table, idx, protos, g)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


for R, D, P, n_table in ((45056, 100, 20, 60000), (32768, 128, 64, 60000)):
    gen = torch.Generator().manual_seed(R + D + P)
    table = (torch.randn(n_table, D, generator=gen) * 0.5).to(dev).requires_grad_(True)
    protos = torch.randn(P, D, generator=gen).to(dev).requires_grad_(True)
    idx = torch.randint(0, n_table, (R,), generator=gen).to(dev)
    g = (torch.randn(R, P, generator=gen) / R).to(dev)
    for fn in (fused, composed):
        timed(fn, table, idx, protos, g, 10)                          # warm-up: code objects, allocator
    ms = {'fused': [], 'composed': []}
    for _ in range(5):                                                # alternating blocks: drift hits both alike
        ms['fused'].append(timed(fused, table, idx, protos, g, args.reps))
        ms['composed'].append(timed(composed, table, idx, protos, g, args.reps))
    row = {'bench': 'proto_sim_fwd_bwd', 'R': R, 'D': D, 'P': P, 'algorithmic_bytes_per_direction': R * D * 4,
           'fused_bytes_moved': moved_fused(R, D, P), 'composed_bytes_moved': moved_composed(R, D, P)}
    for k, v in ms.items():
        row[f'{k}_ms'] = round(float(np.median(v)), 5)
        row[f'{k}_ms_spread'] = [round(min(v), 5), round(max(v), 5)]
    row['fused_over_composed'] = round(row['fused_ms'] / row['composed_ms'], 3)
    row['note'] = 'host-launched autograd round trip, dense table gradient (zero fill + scatter) included in both'
    print(json.dumps(row), flush=True)
