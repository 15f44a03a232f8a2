"""``ops.UniformityFn`` (sbr_uniformity_fwd / sbr_uniformity_bwd) beside torch's own composition of the same term,
``pdist(x).pow(2).mul(-t).exp().mean().log()``, on the same card: loss plus gradient of one side for unit rows at n = 256, 4,096 and
8,192 with D = 64 and 128, t = 2. The kernel must agree with the Gram form of the term in float64 on the device, on the loss within 1e-4
and on the gradient within 1e-4 of its largest element, or the step fails; the pdist route's differences to float64 are reported. Then one
``Trainer`` epoch of ``directau`` (``rec_loss = align``, gamma = 1, D = 64, batch 8,192) on the ML-1M-shaped synthetic world (6,040 x 3,706, 1,000,209 pairs drawn, 3 negatives) beside ``mf`` with bpr on the same world: wall time of
the second epoch (the first warms up) and both epochs' loss figures. Device-event times for the kernels, one warm-up, then the median of
--reps runs; every step runs in a child process under --step-timeout seconds, and after a step that fails or runs out of time no further
step is started. Prints one JSON line. Stand-alone: nothing is gated on these figures.

    python tools/time_directau.py [--reps 7] [--step-timeout 240]
"""
import argparse
import json
import os
import subprocess
import sys
import time

SIDES = [(n, d) for n in (256, 4096, 8192) for d in (64, 128)]
STEPS = [f'side_{n}_{d}' for n, d in SIDES] + ['epoch_directau', 'epoch_mf']
T = 2.0


def _package():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import sibrar_amd as S
    return S


def side(n, d, reps):
    import torch
    S = _package()
    from time_als import timed
    dev = torch.device('cuda:0')
    x = torch.nn.functional.normalize(torch.randn(n, d, device=dev, generator=torch.Generator(device=dev).manual_seed(1)), dim=-1)

    def kernel():
        v = x.detach().requires_grad_()
        S.ops.UniformityFn.apply(v, T).backward()
        return v

    def composed():
        v = x.detach().requires_grad_()
        torch.pdist(v).pow(2).mul(-T).exp().mean().log().backward()
        return v

    # the check: the same term from the Gram form in float64 on the device. The kernel must agree with it; what torch's pdist route
    # gives is reported beside it (its index arithmetic is fp32, and the step does not fail on torch's account)
    def truth():
        v = x.double().requires_grad_()
        sq = (v * v).sum(-1)
        d2 = (sq[:, None] + sq[None, :] - 2 * v @ v.t()).clamp_min(0)
        iu = torch.triu_indices(n, n, 1, device=dev)
        loss = torch.exp(-T * d2[iu[0], iu[1]]).mean().log()
        loss.backward()
        return float(loss), v.grad

    want, want_grad = truth()
    a, b = kernel(), composed()
    la, lb = S.ops.uniformity(x, T)[0], torch.pdist(x).pow(2).mul(-T).exp().mean().log()
    scale = float(want_grad.abs().max())
    d_loss, d_grad = abs(float(la) - want), float((a.grad.double() - want_grad).abs().max()) / scale
    p_loss, p_grad = abs(float(lb) - want), float((b.grad.double() - want_grad).abs().max()) / scale
    del want_grad
    if not (d_loss <= 1e-4 and d_grad <= 1e-4):
        raise SystemExit(f'the kernel disagrees with float64: loss by {d_loss}, gradient by {d_grad} of its largest element')
    print(json.dumps({'step': f'side_{n}_{d}', 'n': n, 'D': d, 't': T, 'loss_float64': want, 'kernel_loss_diff': d_loss, 'kernel_grad_rel_diff': d_grad,
                      'torch_pdist_loss_diff': p_loss, 'torch_pdist_grad_rel_diff': p_grad,
                      'fwd_bwd_ms': {'kernel': timed(kernel, reps), 'torch_pdist': timed(composed, reps)},
                      'fwd_ms': {'kernel': timed(lambda: S.ops.uniformity(x, T), reps),
                                 'torch_pdist': timed(lambda: torch.pdist(x).pow(2).mul(-T).exp().mean().log(), reps)},
                      'device': torch.cuda.get_device_name(0)}))


def epoch(alg):
    import torch
    S = _package()
    S.reproducible(5, deterministic=False)
    ds = S.SyntheticDataset(6040, 3706, 1000209, seed=3, n_negative_samples=3)
    if alg == 'directau':
        net = S.ALGORITHMS['directau'].build_from_conf({'embedding_dim': 64, 'gamma': 1.0, 't': T}, ds)
        loss = S.RecAlignmentLoss(n_items=ds.n_items, neg_train=3)
    else:
        net = S.SGDMatrixFactorization(ds.n_users, ds.n_items, 64)
        loss = S.RecBayesianPersonalizedRankingLoss(n_items=ds.n_items, neg_train=3)
    loader = S.NegativeSamplingDataLoader(ds, batch_size=8192, shuffle=True)
    conf = {'learn': {'lr': 1e-3, 'wd': 0., 'optimizer': 'adam', 'max_batches_per_epoch': len(loader.rows) // 8192},
            'run_settings': {'device': 'cuda:0'}}
    tr = S.Trainer(net, loader, None, loss, conf)
    out = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        figures = tr.train()
        torch.cuda.synchronize()
        out.append({'wall_s': time.perf_counter() - t0, **figures})
    print(json.dumps({'step': f'epoch_{alg}', 'batches': len(loader.rows) // 8192, 'batch': 8192, 'first_epoch': out[0], 'second_epoch': out[1],
                      'device': torch.cuda.get_device_name(0)}))


def step(name, reps):
    kind, *rest = name.split('_')
    return side(int(rest[0]), int(rest[1]), reps) if kind == 'side' else epoch(rest[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--step-timeout', type=float, default=240., help='seconds one step may take')
    ap.add_argument('--step', metavar='NAME', help='run one step in this process (what the parent starts)')
    args = ap.parse_args()
    if args.step:
        return step(args.step, args.reps)
    runs = []
    for name in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), '--reps', str(args.reps), '--step', name]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            runs.append({'step': name, 'error': f'no result within {args.step_timeout:.0f} s'})
            print(json.dumps({'bench': 'directau', 'reps': args.reps, 'runs': runs, 'stopped': True}))
            return 1
        if done.returncode != 0:
            runs.append({'step': name, 'error': f'exit status {done.returncode}', 'stderr': done.stderr[-400:]})
            print(json.dumps({'bench': 'directau', 'reps': args.reps, 'runs': runs, 'stopped': True}))
            return 1
        runs.append(json.loads(done.stdout.strip().splitlines()[-1]))
    print(json.dumps({'bench': 'directau', 'reps': args.reps, 'runs': runs}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
