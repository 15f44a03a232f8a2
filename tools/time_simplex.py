"""Times SimpleX's kernels on the GPU: the cosine contrastive loss with both gradients (``ops.CCLLossFn``, forward and
backward, H [B, D] and the item table as leaves) beside the torch composition of the same step on the same card (gather of the
[B, 1 + N, D] item rows, ``F.cosine_similarity``, ``relu``, autograd with ``index_add``), at B = 1024, D = 64 and N = 100 / 1,000 on the
ML-1M-shaped table (6,040 x 3,706); and one training epoch of the model (the ML-1M-shaped synthetic world of tools/time_directau.py,
1,000,209 pairs drawn, batch 1024, N = 100, Adam through ``FusedOptimizer``). Device events, one warm-up, the median of ``--reps``; the
epoch is timed once by the wall clock after a warm-up of ``--warm`` steps. Prints one JSON line; times in milliseconds.

    python tools/time_simplex.py [--reps 7] [--no-epoch]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = 'cuda'
B, D = 1024, 64
MARGIN, NEGW = 0.9, 10.


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


def torch_step(H, V, i, margin):
    F = torch.nn.functional
    y = F.cosine_similarity(H[:, None, :], V[i], dim=-1)
    return ((1 - y[:, 0]) + NEGW * F.relu(y[:, 1:] - margin).mean(1)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warm', type=int, default=5)
    ap.add_argument('--no-epoch', action='store_true')
    args = ap.parse_args()
    import sibrar_amd as S
    g = torch.Generator().manual_seed(0)
    H = torch.randn(B, D, generator=g).to(DEV).requires_grad_(True)
    V = torch.randn(3706, D, generator=g).to(DEV).requires_grad_(True)
    runs = {'reps': args.reps}
    # random rows have cosines near 0: a margin of 0 keeps about half the negatives active, the paper's 0.9 almost none
    for N in (100, 1000):
        i = torch.randint(0, 3706, (B, 1 + N), generator=g).to(DEV)
        for margin in (0.0, MARGIN):

            def hip_step():
                H.grad = V.grad = None
                loss, _, _ = S.ops.CCLLossFn.apply(H, V, i, margin, NEGW)
                loss.backward()
                return loss

            def hip_fwd():
                with torch.no_grad():
                    return S.ops.CCLLossFn.apply(H, V, i, margin, NEGW)[0]

            def composed():
                H.grad = V.grad = None
                loss = torch_step(H, V, i, margin)
                loss.backward()
                return loss

            a, b = float(hip_step().detach()), float(composed().detach())
            runs[f'N{N}_margin{margin}'] = {'hip_loss_and_gradients_ms': timed(hip_step, args.reps), 'hip_forward_launch_ms': timed(hip_fwd, args.reps),
                                            'torch_composition_ms': timed(composed, args.reps), 'loss_hip': a, 'loss_torch': b}
    if not args.no_epoch:
        S.reproducible(0, deterministic=False)
        ds = S.SyntheticDataset(6040, 3706, 1000209, seed=0, n_negative_samples=100)
        net = S.SimpleX(6040, 3706, ds.user_sampling_matrix_train, embedding_dim=D, init_std=0.1).to(DEV).train()
        opt = S.FusedOptimizer(net, 'adam', 1e-3, 0.)
        none = S.RecNoLoss(n_items=3706)
        loader = S.NegativeSamplingDataLoader(ds, batch_size=B, shuffle=True)
        steps, t0, first, last = 0, None, None, None
        for u, i, _ in loader:
            if steps == args.warm:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            scores = net(u.to(DEV), i.to(DEV))
            other = net.get_and_reset_other_loss()
            (none.compute_loss(scores, None) + other['reg_loss']).backward()
            opt.step()
            opt.zero_grad()
            last = other['reg_loss']
            first = last if first is None else first
            steps += 1
        torch.cuda.synchronize()
        if t0 is None:
            raise SystemExit(f'the epoch has {steps} steps, no more than the {args.warm} warm-up steps: nothing was timed')
        wall = time.perf_counter() - t0
        runs['epoch'] = {'steps': steps, 'timed_steps': steps - args.warm, 'ms_per_step_with_the_loader': 1e3 * wall / max(steps - args.warm, 1),
                         'epoch_s_extrapolated': wall / max(steps - args.warm, 1) * steps, 'loss_first': float(first), 'loss_last': float(last)}
    print(json.dumps({'bench': 'simplex', 'B': B, 'D': D, **runs}))


if __name__ == '__main__':
    main()
