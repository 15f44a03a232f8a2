"""One layer of SimGCL / XSimGCL per launch: ``ops.graph_propagate_noise`` (sbr_graph_propagate_noise_f32: propagation, perturbation and
running sum in one launch, the noise made in registers) beside the composition it replaces on the same card — ``ops.graph_propagate``,
then torch's ``rand_like``, ``normalize``, ``sign``, multiply, add, and a separate update of the running sum — and beside the clean launch
``ops.graph_propagate`` with its sum epilogue, which is the floor: what the fused launch adds to it is the price of the noise. The graph
is the ML-1M-shaped synthetic world of tools/time_directau.py (6,040 x 3,706, 1,000,209 pairs drawn) and one ten times smaller, D = 64.

Before anything is timed the fused launch is checked on the device: eps = 0 gives the clean launch's bits, and a row's perturbation has
length eps within 1e-5 (fp32 rounding of a 64-term norm and of the final addition) wherever the clean row has no zero; otherwise the
step fails. The two routes draw different noise, so their outputs are not compared. Timing: device events around ``--inner`` launches
in a row (one launch alone is a few tens of microseconds: mostly the clock), one warm-up window, then ``--reps`` windows per route with
the routes alternating; the median and the spread (minimum, maximum) per launch are reported, and the table passes each route makes
over [n_users + n_items, D] beside the gather, counted from the code. Every step runs in a child process under --step-timeout seconds,
and after a step that fails or runs out of time no further step is started. Prints one JSON line. Stand-alone: nothing is gated on
these figures.

    python tools/time_simgcl.py [--reps 9] [--inner 50] [--step-timeout 240]
"""
import argparse
import json
import os
import subprocess
import sys

WORLDS = {'ml1m': (6040, 3706, 1000209), 'tenth': (604, 371, 100021)}
D, EPS = 64, 0.1
# whole-table passes (reads + writes of [n, D] fp32) on top of the neighbour gather, counted from the code of each route
PASSES = {'fused': 'write y, read sum, write sum: 3',
          'clean': 'write y, read sum, write sum: 3',
          'composed': 'write y; rand_like: 1 write; sign: 1 read, 1 write; normalize: 2 reads, 1 write; two multiplies (eps a scalar): '
                      '3 reads, 2 writes; add_: 2 reads, 1 write; sum update: 2 reads, 1 write: 18'}


def _package():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import sibrar_amd as S
    return S


def step(name, reps, inner):
    import numpy as np
    import torch
    S = _package()
    from importlib import import_module
    features = import_module(S.ops.__name__.rsplit('.', 1)[0] + '.features')
    dev = torch.device('cuda:0')
    n_users, n_items, pairs = WORLDS[name]
    ds = S.SyntheticDataset(n_users, n_items, pairs, seed=3, n_negative_samples=3)
    csr = features.DeviceCSR(ds.user_sampling_matrix_train).to(dev)
    n = n_users + n_items
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(n, D, device=dev, generator=gen) / 4
    y, acc = torch.empty_like(x), torch.zeros_like(x)
    ops = S.ops

    def fused():
        ops.graph_propagate_noise(csr, x, EPS, 7, 3, out=y, sum=acc, sum_scale=1.0)

    def clean():
        ops.graph_propagate(csr, x, out=y, sum=acc, sum_scale=1.0)

    def composed():
        ops.graph_propagate(csr, x, out=y)
        noise = torch.rand_like(y)
        y.add_(torch.sign(y) * torch.nn.functional.normalize(noise, dim=-1) * EPS)
        acc.add_(y)                                                             # the running sum: a pass of its own

    # the check
    p = ops.graph_propagate(csr, x)
    z = ops.graph_propagate_noise(csr, x, 0.0, 7, 3)
    if not torch.equal(p.view(torch.int32), z.view(torch.int32)):
        raise SystemExit('eps = 0 differs from the clean launch')
    q = ops.graph_propagate_noise(csr, x, EPS, 7, 3)
    full = (p != 0).all(1)
    length = (q.double() - p.double()).norm(dim=1)[full]
    worst = float((length - float(np.float32(EPS))).abs().max())
    if not (bool(full.any()) and worst <= 1e-5):
        raise SystemExit(f"a row's perturbation misses the length eps by {worst}")

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / inner                                  # microseconds per launch (per layer)

    routes = {'fused': fused, 'composed': composed, 'clean': clean}
    for fn in routes.values():
        window(fn)
    times = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            times[k].append(window(fn))
    nnz = int(csr.indices.numel())
    table = 4 * n * D
    out = {'step': name, 'n_users': n_users, 'n_items': n_items, 'nnz': nnz, 'D': D, 'eps': EPS, 'inner': inner,
           'table_bytes': table, 'gather_bytes': 2 * nnz * 4 * D, 'noise_length_worst_diff': worst,
           'us_per_layer': {k: {'median': float(np.median(v)), 'min': float(np.min(v)), 'max': float(np.max(v))} for k, v in times.items()},
           'table_passes': PASSES, 'device': torch.cuda.get_device_name(0)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=50, help='launches per timed window')
    ap.add_argument('--step-timeout', type=float, default=240., help='seconds one step may take')
    ap.add_argument('--step', metavar='NAME', help='run one step in this process (what the parent starts)')
    args = ap.parse_args()
    if args.step:
        return step(args.step, args.reps, args.inner)
    runs = []
    for name in WORLDS:
        cmd = [sys.executable, os.path.abspath(__file__), '--reps', str(args.reps), '--inner', str(args.inner), '--step', name]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            runs.append({'step': name, 'error': f'no result within {args.step_timeout:.0f} s'})
            print(json.dumps({'bench': 'simgcl', 'reps': args.reps, 'runs': runs, 'stopped': True}))
            return 1
        if done.returncode != 0:
            runs.append({'step': name, 'error': f'exit status {done.returncode}', 'stderr': done.stderr[-400:]})
            print(json.dumps({'bench': 'simgcl', 'reps': args.reps, 'runs': runs, 'stopped': True}))
            return 1
        runs.append(json.loads(done.stdout.strip().splitlines()[-1]))
    print(json.dumps({'bench': 'simgcl', 'reps': args.reps, 'runs': runs}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
