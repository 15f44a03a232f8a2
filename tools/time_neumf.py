"""Times NeuMF's evaluation kernel on the GPU: ``ops.neumf_score_all`` beside the torch composition of the same scores
(``relu(A[:, None] + Bt[None])``, the tail layers as matmuls, in user chunks whose [chunk, I, H] activation stays under 1 GiB) at
6,040 x 3,706 and at 100,000 x 50,000, with the tails (32, 16, 8) and (64, 64, 64, 64); and one full
``evaluate_recommender_algorithm(scorer='fp32')`` of the default model on the ML-1M-shaped synthetic world beside ``mf``'s at
``embedding_dim`` 64. At the large size one chunk of ``--chunk`` users is timed on either side and the whole is that time scaled by the
number of chunks (``extrapolated`` in the output). Every GPU step runs in a child process under its own time limit; the first step that
fails or runs out of time is reported (``stopped`` names it), no further step is started and the exit status is 1. Device events, one
warm-up, the median of ``--reps``. Prints one JSON line; times in milliseconds.

    python tools/time_neumf.py [--reps 5] [--chunk 4096] [--limit 240]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = 'cuda'
SIZES = {'ml1m': (6040, 3706), 'c2': (100000, 50000)}
TAILS = {'default': (32, 16, 8), 'caps': (64, 64, 64, 64)}


def timed(fn, reps):
    import torch
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


def step_score(size, tail, reps, chunk):
    import torch
    import sibrar_amd as S
    Bu, I = SIZES[size]
    widths = TAILS[tail]
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    n_u = min(Bu, chunk)
    A, Bt = r(n_u, widths[0]), r(I, widths[0])
    Ws = [r(widths[l], widths[l - 1]) / widths[l - 1] ** 0.5 for l in range(1, len(widths))]
    bs = [0.1 * r(widths[l]) for l in range(1, len(widths))]
    w_h, c = r(widths[-1]), r(1)
    packed = S.ops.neumf_pack_tail(Ws, bs, w_h, c)
    out = torch.empty(n_u, I, device=DEV)
    hip = timed(lambda: S.ops.neumf_score_all(A, Bt, packed, widths, out=out), reps)
    rows = max(1, min(n_u, (1 << 28) // (I * max(widths))))       # [rows, I, H] floats under 1 GiB
    ref = torch.empty(rows, I, device=DEV)

    def composed():
        z = torch.relu(A[:rows, None, :] + Bt[None])
        for W, b in zip(Ws, bs):
            z = torch.relu(z @ W.t() + b)
        torch.add(z @ w_h, c, out=ref)

    tc = timed(composed, reps)
    err = float((out[:rows] - ref).abs().max())
    scale, fmas = Bu / n_u, sum(widths[l] * widths[l - 1] for l in range(1, len(widths))) + widths[-1]
    return {'users_timed': n_u, 'hip_ms': hip, 'hip_whole_ms': hip * scale, 'extrapolated': n_u < Bu, 'torch_rows_per_chunk': rows,
            'torch_chunk_ms': tc, 'torch_whole_ms': tc * Bu / rows, 'max_abs_difference': err,
            'hip_tflops': 2e-9 * fmas * n_u * I / hip}


def step_eval(which, reps):
    import torch
    import sibrar_amd as S
    S.reproducible(0, deterministic=False)
    ds = S.SyntheticDataset(6040, 3706, 1000209, seed=0, n_negative_samples=4, holdout_per_user=1)
    net = (S.NeuMF(6040, 3706) if which == 'neumf' else S.SGDMatrixFactorization(6040, 3706, 64)).to(DEV).eval()
    view = ds.eval_view()
    loader = type('L', (), {'dataset': view, 'batch_size': 256})()

    def run():
        ev = S.FullEvaluator(config=S.evaluation._Cfg(top_k=(10,)), dataset=view)
        return S.evaluate_recommender_algorithm(net, loader, ev, device=DEV, scorer='fp32')

    run()
    torch.cuda.synchronize()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        walls.append(1e3 * (time.perf_counter() - t0))
    return {'evaluation_wall_ms': statistics.median(walls)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--chunk', type=int, default=4096)
    ap.add_argument('--limit', type=int, default=240, help='seconds a child may run')
    ap.add_argument('--step', default=None, help='(internal) run one step in this process')
    args = ap.parse_args()
    if args.step is not None:
        kind, *rest = args.step.split(':')
        res = step_score(rest[0], rest[1], args.reps, args.chunk) if kind == 'score' else step_eval(rest[0], args.reps)
        print('RESULT ' + json.dumps(res))
        return
    steps = [f'score:{s}:{t}' for s in SIZES for t in TAILS] + ['eval:neumf', 'eval:mf']
    runs = {'reps': args.reps}
    for step in steps:
        cmd = [sys.executable, os.path.abspath(__file__), '--step', step, '--reps', str(args.reps), '--chunk', str(args.chunk)]
        # a child that fails in any way, or gives no result in time, may have left the card unwell: nothing more is started on it
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            runs[step] = {'failed': f'no result within {args.limit} s'}
            runs['stopped'] = step
            break
        lines = [l for l in done.stdout.splitlines() if l.startswith('RESULT ')]
        if done.returncode != 0 or not lines:
            runs[step] = {'failed': f'exit status {done.returncode}', 'stderr_tail': done.stderr[-400:]}
            runs['stopped'] = step
            break
        runs[step] = json.loads(lines[-1][len('RESULT '):])
    print(json.dumps({'bench': 'neumf', **runs}))
    if 'stopped' in runs:
        sys.exit(1)


if __name__ == '__main__':
    main()
