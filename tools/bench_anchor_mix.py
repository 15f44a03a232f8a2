"""ACF's anchor mixing: ``ops.AnchorMixFn`` (lookup, logits, softmax, mixture and both entropy regularisers in one op each way) against
the composition available without it — ``LookupFn`` -> ``linear_nt`` -> torch ``softmax`` -> ``matmul_nn`` -> torch ``logsumexp`` and
the two entropies, and autograd's mirror image of those in the backward —, one training step's forward + backward at (R, D, K) =
(45056, 100, 20) and (32768, 128, 64): device-event times over alternating repetitions, and the bytes each variant's kernels move
(counted from their loads and stores) against the algorithmic R D 4 per direction. The composition is the baseline, not the code under
test. One JSON line per shape.

    python tools/bench_anchor_mix.py [--reps 100]
"""
import argparse
import json
import math
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
W_EXC, W_INC = 1e-1, 1e-2


def fused(table, idx, anchors, g):
    r, _, exc, inc = ops.AnchorMixFn.apply(table, idx, anchors, True)
    torch.autograd.backward([r, W_EXC * exc + W_INC * inc], [g, None])


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


class _MatmulNN(torch.autograd.Function):
    """c @ a through the library's GEMMs, both gradients"""

    @staticmethod
    def forward(ctx, c, a):
        ctx.save_for_backward(c, a)
        return ops.matmul_nn(c.contiguous(), a)

    @staticmethod
    def backward(ctx, g):
        c, a = ctx.saved_tensors
        g = g.contiguous()
        return ops.linear_nt(g, a), ops.matmul_tn(c.contiguous(), g)


def composed(table, idx, anchors, g):
    e = ops.LookupFn.apply(table, idx)
    s = _LinearNT.apply(e, anchors)
    c = torch.softmax(s, dim=-1)
    r = _MatmulNN.apply(c, anchors)
    exc = (-(c * (s - torch.logsumexp(s, dim=-1, keepdim=True)))).sum(-1).mean()
    q = c.sum(dim=0) / c.sum()
    inc = math.log(anchors.shape[0]) + (q * torch.log(q)).sum()
    torch.autograd.backward([r, W_EXC * exc + W_INC * inc], [g, None])


def moved_fused(R, D, K):
    """bytes of AnchorMixFn's kernels: forward reads the rows once, writes r, c and lse; backward reads G and the rows once for the logits
    and dc and once more per anchor tile for dA (cache hits of the same workgroup's tile, counted all the same), c twice, writes dE and adds
    its dA partial once per row tile; the scatter into the table gradient reads dE and writes the touched rows"""
    rows, ent, tiles, kt = R * D * 4, R * K * 4, -(-R // 64), -(-K // 64)
    fwd = rows + rows + ent + R * 4
    bwd = 2 * rows + kt * 2 * rows + 2 * ent + R * 4 + rows + tiles * 2 * K * D * 4
    scatter = 2 * rows
    return fwd + bwd + scatter


def moved_composed(R, D, K):
    rows, ent = R * D * 4, R * K * 4
    lookup = 2 * rows                                                 # gather: read, write the copy
    gemm1 = rows + ent                                                # s
    softmax = 2 * ent                                                 # read s, write c
    gemm2 = ent + rows                                                # r
    entropies = 2 * ent + (3 * ent + ent) + ent + ent                 # logsumexp, s - lse and its product with c (read 2 + write 1, sum), c.sum(0), c.sum()
    bwd_r = (rows + ent) + (ent + rows)                               # dc = G A^T (read G, write dc), dA += c^T G (read c, G)
    bwd_elementwise = 2 * ent * 5                                     # gradients of the entropy terms, their accumulation into dc and ds
    bwd_softmax = 3 * ent                                             # read c, dc, write ds
    bwd_s = (ent + rows) + (ent + rows)                               # dE = ds A (write rows), dA += ds^T e (read rows)
    scatter = 2 * rows
    return lookup + gemm1 + softmax + gemm2 + entropies + bwd_r + bwd_elementwise + bwd_softmax + bwd_s + scatter


def timed(fn, table, idx, anchors, g, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        table.grad = anchors.grad = None
        fn(table, idx, anchors, g)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


for R, D, K, n_table in ((45056, 100, 20, 60000), (32768, 128, 64, 60000)):
    gen = torch.Generator().manual_seed(R + D + K)
    table = (torch.randn(n_table, D, generator=gen) * 0.5).to(dev).requires_grad_(True)
    anchors = (torch.randn(K, D, generator=gen) * 0.5).to(dev).requires_grad_(True)
    idx = torch.randint(0, n_table, (R,), generator=gen).to(dev)
    g = (torch.randn(R, D, generator=gen) / R).to(dev)
    grads = {}
    for name, fn in (('fused', fused), ('composed', composed)):
        timed(fn, table, idx, anchors, g, 10)                         # warm-up: code objects, allocator
        grads[name] = (table.grad.clone(), anchors.grad.clone())
    # the two variants compute the same gradients (fp32 reorderings apart)
    agree = [float((a - b).norm() / b.norm()) for a, b in zip(grads['fused'], grads['composed'])]
    ms = {'fused': [], 'composed': []}
    for _ in range(5):                                                # alternating blocks: drift hits both alike
        ms['fused'].append(timed(fused, table, idx, anchors, g, args.reps))
        ms['composed'].append(timed(composed, table, idx, anchors, g, args.reps))
    row = {'bench': 'anchor_mix_fwd_bwd', 'R': R, 'D': D, 'K': K, 'algorithmic_bytes_per_direction': R * D * 4,
           'fused_bytes_moved': moved_fused(R, D, K), 'composed_bytes_moved': moved_composed(R, D, K),
           'rel_diff_table_grad': agree[0], 'rel_diff_anchor_grad': agree[1]}
    for k, v in ms.items():
        row[f'{k}_ms'] = round(float(np.median(v)), 5)
        row[f'{k}_ms_spread'] = [round(min(v), 5), round(max(v), 5)]
    row['fused_over_composed'] = round(row['fused_ms'] / row['composed_ms'], 3)
    row['note'] = 'host-launched autograd round trip, dense table gradient (zero fill + scatter) included in both'
    print(json.dumps(row), flush=True)
