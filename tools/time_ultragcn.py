"""Times UltraGCN's kernels on the GPU: the build of the item-item lists (``ops.ultragcn_scales`` +
``ops.cooc_weight_topk``, K = 10) and one training step's loss with both table gradients (``ops.LookupFn`` + ``ops.UltraGCNLossFn``, forward
and backward) beside the torch composition of the same step on the same card (gather of the [B, 1 + N + K, D] item rows, ``bmm``, three
weighted ``binary_cross_entropy_with_logits`` calls, autograd with ``index_add``), at B = 1024, D = 64, K = 10 and N = 300 / 1500 on the
ML-1M-shaped synthetic world of tools/time_directau.py (6,040 x 3,706, 1,000,209 pairs drawn). Device events, one warm-up, the median of
``--reps``. Prints one JSON line; times in milliseconds.

    python tools/time_ultragcn.py [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = 'cuda'
B, D, K = 1024, 64, 10
SC = (1e-6, 1., 1e-6, 1., 300., 5e-4)


def timed(fn, reps):
    fn()                                                          # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def torch_step(U, V, u, i, beta_u, beta_i, nbr_idx, nbr_val, N):
    F = torch.nn.functional
    w1, w2, w3, w4, negw, lam = SC
    p = i[:, 0]
    nb = nbr_idx[p].long()
    mask = nb >= 0
    items = torch.cat([i, nb.clamp(min=0)], 1)
    s = torch.bmm(V[items], U[u][:, :, None])[:, :, 0]
    bu = beta_u[u][:, None]
    pos = F.binary_cross_entropy_with_logits(s[:, 0], torch.ones_like(s[:, 0]), weight=w1 + w2 * bu[:, 0] * beta_i[p], reduction='sum')
    neg = F.binary_cross_entropy_with_logits(s[:, 1:1 + N], torch.zeros_like(s[:, 1:1 + N]), weight=w3 + w4 * bu * beta_i[i[:, 1:]],
                                             reduction='none').mean(1).sum()
    nbr = F.binary_cross_entropy_with_logits(s[:, 1 + N:], torch.ones_like(s[:, 1 + N:]), weight=nbr_val[p] * mask, reduction='sum')
    return pos + negw * neg + lam * nbr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    args = ap.parse_args()
    import sibrar_amd as S
    from importlib import import_module
    features = import_module(S.ops.__name__.rsplit('.', 1)[0] + '.features')
    ds = S.SyntheticDataset(6040, 3706, 1000209, seed=0, n_negative_samples=4)
    csr = features.DeviceCSR(ds.user_sampling_matrix_train).to(DEV)
    csr.transposed()
    runs = {'reps': args.reps, 'nnz': int(csr.indices.numel())}

    def build():
        beta_u, beta_i, row, col = S.ops.ultragcn_scales(csr)
        return (beta_u, beta_i) + S.ops.cooc_weight_topk(csr, row, col, K)

    runs['list_build_ms'] = timed(build, args.reps)
    runs['scales_ms'] = timed(lambda: S.ops.ultragcn_scales(csr), args.reps)
    beta_u, beta_i, nbr_idx, nbr_val, nbr_len = build()
    g = torch.Generator().manual_seed(0)
    U = (torch.randn(6040, D, generator=g) * 0.1).to(DEV).requires_grad_(True)
    V = (torch.randn(3706, D, generator=g) * 0.1).to(DEV).requires_grad_(True)
    for N in (300, 1500):
        u = torch.randint(0, 6040, (B,), generator=g).to(DEV)
        i = torch.randint(0, 3706, (B, 1 + N), generator=g).to(DEV)

        def hip_step():
            U.grad = V.grad = None
            loss, _, _ = S.ops.UltraGCNLossFn.apply(S.ops.LookupFn.apply(U, u), V, u, i, beta_u, beta_i, nbr_idx, nbr_val, nbr_len, *SC)
            loss.backward()
            return loss

        def hip_fwd():
            with torch.no_grad():
                return S.ops.UltraGCNLossFn.apply(S.ops.LookupFn.apply(U, u), V, u, i, beta_u, beta_i, nbr_idx, nbr_val, nbr_len, *SC)[0]

        def composed():
            U.grad = V.grad = None
            loss = torch_step(U, V, u, i, beta_u, beta_i, nbr_idx, nbr_val, N)
            loss.backward()
            return loss

        a, b = float(hip_step().detach()), float(composed().detach())
        runs[f'N{N}'] = {'hip_loss_and_gradients_ms': timed(hip_step, args.reps), 'hip_forward_launch_ms': timed(hip_fwd, args.reps),
                         'torch_composition_ms': timed(composed, args.reps), 'loss_hip': a, 'loss_torch': b}
    print(json.dumps({'bench': 'ultragcn', 'B': B, 'D': D, 'K': K, **runs}))


if __name__ == '__main__':
    main()
