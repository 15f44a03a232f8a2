"""PopularItems' top-100 lists for every user of a synthetic split at ML-1M's shape (6,040 users x 3,706 items, 946,068 interactions) and
at 100,000 x 50,000 with 5,000,000 interactions, the exclusions being the training interactions of ``SyntheticDataset``: the walk over the
shared ranking (``PopularItems.topk_lists`` -> ``ops.shared_rank_topk``) in the evaluation's 16,384-user chunks and in one call, and beside it
the composition of the ops the evaluation used before — the score row expanded to [chunk, items], ``ops.mask_scores_``, ``ops.topk_rows`` —
in the same chunks. Device-event times, one warm-up, then the median of --reps runs. Every (shape, route) step runs in a child process of
its own under --step-timeout seconds; after a step that fails or runs out of time no further step is started. Prints one JSON line.
Stand-alone: nothing is gated on these figures.

    python tools/time_naive.py [--reps 7] [--small] [--step-timeout 240]
"""
import argparse
import json
import os
import subprocess
import sys

K = 100
CHUNK = 16384
SHAPES = {'ml1m': (6040, 3706, 946068), 'c2': (100000, 50000, 5000000)}
ROUTES = ('walk', 'composition')


def step(shape, route, reps):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import sibrar_amd as S
    from time_als import timed

    n_users, n_items, nnz = SHAPES[shape]
    dev = torch.device('cuda:0')
    ds = S.SyntheticDataset(n_users, n_items, nnz, item_popularity=1.0)
    excl = ds.user_sampling_matrix_train.tocsr()
    excl.sort_indices()
    indptr = torch.from_numpy(excl.indptr.astype(np.int64)).to(dev)
    indices = torch.from_numpy(excl.indices.astype(np.int32)).to(dev)
    alg = S.PopularItems.build_from_conf({}, ds).to(dev)
    items = torch.arange(n_items, device=dev)
    users = torch.arange(n_users, device=dev)
    chunks = [users[s:s + CHUNK] for s in range(0, n_users, CHUNK)]
    res = {'shape': shape, 'route': route, 'n_users': n_users, 'n_items': n_items, 'nnz': int(excl.nnz), 'k': K, 'chunk': CHUNK}

    def walk(parts):
        return [alg.topk_lists(u, items, indptr, indices, K) for u in parts]

    def composition():
        out = []
        for u in chunks:
            rows = alg.combine_user_item_representations(u, (items,))
            S.ops.mask_scores_(rows, u, indptr, indices)
            out.append(S.ops.topk_rows(rows, K))
        return out

    if route == 'walk':
        score = alg.pop_distribution.to(dev)
        res['ranking_ms'] = timed(lambda: S.ops.shared_ranking(score), reps)
        res['walk_chunked_ms'] = timed(lambda: walk(chunks), reps)
        res['walk_one_call_ms'] = timed(lambda: walk([users]), reps)
        res['score_bytes_of_the_composition'] = 4 * n_users * n_items
    else:
        res['composition_ms'] = timed(composition, reps)
        a, b = walk(chunks), composition()
        res['same_lists'] = all(torch.equal(x[1], y[1]) and bool((x[0] == y[0]).all()) for x, y in zip(a, b))
    res['device'] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--small', action='store_true', help="ML-1M's shape only")
    ap.add_argument('--step-timeout', type=float, default=240., help='seconds one (shape, route) step may take')
    ap.add_argument('--step', nargs=2, metavar=('SHAPE', 'ROUTE'), help='run one step in this process (what the parent starts)')
    args = ap.parse_args()
    if args.step:
        return step(args.step[0], args.step[1], args.reps)
    runs = []
    for shape in (('ml1m',) if args.small else tuple(SHAPES)):
        for route in ROUTES:
            cmd = [sys.executable, os.path.abspath(__file__), '--reps', str(args.reps), '--step', shape, route]
            try:
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                runs.append({'shape': shape, 'route': route, 'error': f'no result within {args.step_timeout:.0f} s'})
                print(json.dumps({'bench': 'naive', 'k': K, 'reps': args.reps, 'runs': runs, 'stopped': True}))
                return 1
            if done.returncode != 0:
                runs.append({'shape': shape, 'route': route, 'error': f'exit status {done.returncode}', 'stderr': done.stderr[-400:]})
                print(json.dumps({'bench': 'naive', 'k': K, 'reps': args.reps, 'runs': runs, 'stopped': True}))
                return 1
            runs.append(json.loads(done.stdout.strip().splitlines()[-1]))
    print(json.dumps({'bench': 'naive', 'k': K, 'reps': args.reps, 'runs': runs}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
