"""``ops.rank_metrics_pos`` (sbr_rank_metrics_pos: dcg, ap, rr, one wave per user) beside ``ops.rank_metrics`` (sbr_rank_metrics: ndcg,
recall, precision, one thread per user) on the same lists: 100,000 users and ML-1M's 6,040, lists of 100 random distinct items of a
catalogue of 50,000 / 3,706, 20 random labels per user of which 5 are planted in the list, the reference's seven cut-offs. The two kernels
compute different metrics: the comparison shows what the walk costs, it is no speed-up claim. Device-event times, one warm-up, then
the median of --reps runs, each shape in a child process under --step-timeout seconds; after a step that fails or runs out of time no
further step is started. Prints one JSON line. Stand-alone: nothing is gated on these figures.

    python tools/time_rank_pos.py [--reps 7] [--step-timeout 240]
"""
import argparse
import json
import os
import subprocess
import sys

KS = [1, 3, 5, 10, 20, 50, 100]
SHAPES = {'ml1m': (6040, 3706), 'c2': (100000, 50000)}


def step(shape, reps):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import sibrar_amd as S
    from time_als import timed

    n_users, n_items = SHAPES[shape]
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(7)
    order = torch.rand(n_users, n_items, device=dev, generator=g).argsort(dim=1)
    top = order[:, :100].to(torch.int32).contiguous()
    labels = torch.cat([order[:, 100:115], order[:, torch.tensor([0, 7, 30, 64, 99], device=dev)]], dim=1).sort(dim=1)[0]
    del order
    indptr = (torch.arange(n_users + 1, device=dev, dtype=torch.int64) * labels.shape[1]).contiguous()
    indices = labels.reshape(-1).to(torch.int32).contiguous()
    users = torch.arange(n_users, device=dev, dtype=torch.int64)
    res = {'shape': shape, 'n_users': n_users, 'n_items': n_items, 'kmax': 100, 'ks': KS, 'labels_per_user': int(labels.shape[1]),
           'rank_metrics_ms': timed(lambda: S.ops.rank_metrics(top, users, indptr, indices, KS), reps),
           'rank_metrics_pos_ms': timed(lambda: S.ops.rank_metrics_pos(top, users, indptr, indices, KS), reps)}
    rr = S.ops.rank_metrics_pos(top, users, indptr, indices, KS)[2]
    res['every_rr_is_one'] = bool((rr == 1).all())               # rank 0 is planted: the lists and labels are what the text says
    res['device'] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--step-timeout', type=float, default=240., help='seconds one shape may take')
    ap.add_argument('--step', metavar='SHAPE', help='run one shape in this process (what the parent starts)')
    args = ap.parse_args()
    if args.step:
        return step(args.step, args.reps)
    runs = []
    for shape in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), '--reps', str(args.reps), '--step', shape]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            runs.append({'shape': shape, 'error': f'no result within {args.step_timeout:.0f} s'})
            print(json.dumps({'bench': 'rank_pos', 'reps': args.reps, 'runs': runs, 'stopped': True}))
            return 1
        if done.returncode != 0:
            runs.append({'shape': shape, 'error': f'exit status {done.returncode}', 'stderr': done.stderr[-400:]})
            print(json.dumps({'bench': 'rank_pos', 'reps': args.reps, 'runs': runs, 'stopped': True}))
            return 1
        runs.append(json.loads(done.stdout.strip().splitlines()[-1]))
    print(json.dumps({'bench': 'rank_pos', 'reps': args.reps, 'runs': runs}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
