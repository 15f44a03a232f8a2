"""``ops.graph_propagate`` / ``ops.LightGCNPropagateFn`` (sbr_graph_propagate_f32) beside two other ways to the same numbers on the same
card: the composition the package could already do (``ops.csr_times_dense`` per side plus torch's scalings and adds) and
``torch.sparse.mm`` on the normalised adjacency as a sparse CSR tensor. Two shapes, D = 64: ML-1M's dimensions, 6,040 x 3,706, and
100,000 x 25,000, items drawn by a Zipf(1) popularity (long item rows). The generator draws 1,000,209 and 5,000,000 pairs and keeps the
distinct ones: 588,453 and 3,931,731 entries, so the first shape has ML-1M's dimensions at about 60 % of its density, not its data.
Timed: one propagation layer with the running sum ``sum = (sum + y) / 2`` (fused in the kernel, torch operators on the other two routes;
the factor keeps the sum bounded over the repetitions), and a whole L = 3 forward plus backward. The three routes must agree on the
L = 3 mean within 1e-5 (values of the order 0.1, fp32 sums in different orders); the step fails otherwise. Device-event times, one warm-up,
then the median of --reps runs, each shape in a child process under --step-timeout seconds; after a step that fails or runs out of time
no further step is started. Prints one JSON line. Stand-alone: nothing is gated on these figures.

    python tools/time_lightgcn.py [--reps 7] [--step-timeout 240]
"""
import argparse
import json
import os
import subprocess
import sys

SHAPES = {'ml1m': (6040, 3706, 1000209), 'c2': (100000, 25000, 5000000)}
D, LAYERS = 64, 3


def step(shape, reps):
    from types import SimpleNamespace
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import sibrar_amd as S
    from importlib import import_module
    from time_als import timed
    pkg = S.ops.__name__.rsplit('.', 1)[0]
    features, datasets = import_module(pkg + '.features'), import_module(pkg + '.datasets')

    n_users, n_items, nnz = SHAPES[shape]
    dev = torch.device('cuda:0')
    m = datasets.synthetic_interactions(n_users, n_items, nnz, seed=3, item_popularity=1.0)
    csr = features.DeviceCSR(m).to(dev)
    t_indptr, t_indices, _ = csr.transposed()
    side_t = SimpleNamespace(shape=(n_items, n_users), indptr=t_indptr, indices=t_indices, data=None)
    n = n_users + n_items
    deg = torch.cat([csr.indptr[1:] - csr.indptr[:-1], t_indptr[1:] - t_indptr[:-1]]).float()
    s = torch.where(deg > 0, 1.0 / deg.sqrt(), torch.zeros_like(deg))[:, None]
    e0 = torch.randn(n, D, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) / 8
    grad = torch.randn(n, D, device=dev, generator=torch.Generator(device=dev).manual_seed(2)) / 8

    # 1. the kernel
    out, acc = torch.empty_like(e0), e0.clone()
    ops = S.ops

    def kernel_layer():
        ops.graph_propagate(csr, e0, out=out, sum=acc, sum_scale=0.5)

    def kernel_model():
        x = e0.detach().requires_grad_()
        ops.LightGCNPropagateFn.apply(csr, x, LAYERS).backward(grad)

    # 2. the composition from ops.csr_times_dense: scale, one product per side, scale, add
    def composed_layer(x=e0, total=acc, scale=0.5):
        z = s * x
        y = torch.empty_like(x)
        ops.csr_times_dense(csr, z[n_users:], out=y[:n_users])
        ops.csr_times_dense(side_t, z[:n_users], out=y[n_users:])
        y *= s
        total += y
        if scale != 1.0:
            total *= scale
        return y

    def composed_mean(x):
        total = x.clone()
        for k in range(1, LAYERS + 1):
            x = composed_layer(x, total, 1.0 if k < LAYERS else 1.0 / (LAYERS + 1))
        return total

    def composed_model():                                          # the operator is symmetric: backward is the same mean on the gradient
        composed_mean(e0)
        composed_mean(grad)

    # 3. torch.sparse.mm on A^ as a sparse CSR tensor
    a = sp_adjacency(m, s.cpu().numpy()[:, 0], dev)

    def or_error(fn):
        try:
            return timed(fn, reps)
        except RuntimeError as e:                                  # a torch build without this sparse product or its gradient
            return f'{type(e).__name__}: {str(e)[:120]}'

    def sparse_layer():
        y = torch.sparse.mm(a, e0)
        acc.add_(y).mul_(0.5)

    def sparse_mean(x):
        total, y = x, x
        for _ in range(LAYERS):
            y = torch.sparse.mm(a, y)
            total = total + y
        return total / (LAYERS + 1)

    def sparse_model():
        sparse_mean(e0.detach().requires_grad_()).backward(grad)

    want = ops.LightGCNPropagateFn.apply(csr, e0, LAYERS)
    diffs = {'csr_times_dense': float((composed_mean(e0) - want).abs().max())}
    try:
        diffs['torch_sparse_mm'] = float((sparse_mean(e0) - want).abs().max())
    except RuntimeError as e:
        diffs['torch_sparse_mm'] = f'{type(e).__name__}: {str(e)[:120]}'
    worst = max(v for v in diffs.values() if isinstance(v, float))
    if not worst <= 1e-5:
        raise SystemExit(f'the routes disagree on the L = {LAYERS} mean: {diffs}')
    res = {'shape': shape, 'n_users': n_users, 'n_items': n_items, 'nnz': int(m.nnz), 'D': D, 'layers': LAYERS,
           'longest_row': int(deg.max()),
           'max_diff_to_kernel': diffs,
           'layer_ms': {'kernel': timed(kernel_layer, reps), 'csr_times_dense': timed(composed_layer, reps), 'torch_sparse_mm': or_error(sparse_layer)},
           'model_fwd_bwd_ms': {'kernel': timed(kernel_model, reps), 'csr_times_dense': timed(composed_model, reps),
                                'torch_sparse_mm': or_error(sparse_model)},
           'device': torch.cuda.get_device_name(0)}
    print(json.dumps(res))


def sp_adjacency(m, s, dev):
    import numpy as np
    import scipy.sparse as sp
    import torch
    a = sp.bmat([[None, m], [m.T, None]], format='csr').astype(np.float32)
    a = sp.csr_matrix(sp.diags(s) @ a @ sp.diags(s)).astype(np.float32)
    a.sort_indices()
    return torch.sparse_csr_tensor(torch.from_numpy(a.indptr.astype(np.int64)), torch.from_numpy(a.indices.astype(np.int64)),
                                   torch.from_numpy(a.data), size=a.shape).to(dev)


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
            print(json.dumps({'bench': 'lightgcn', 'reps': args.reps, 'runs': runs, 'stopped': True}))
            return 1
        if done.returncode != 0:
            runs.append({'shape': shape, 'error': f'exit status {done.returncode}', 'stderr': done.stderr[-400:]})
            print(json.dumps({'bench': 'lightgcn', 'reps': args.reps, 'runs': runs, 'stopped': True}))
            return 1
        runs.append(json.loads(done.stdout.strip().splitlines()[-1]))
    print(json.dumps({'bench': 'lightgcn', 'reps': args.reps, 'runs': runs}))
    return 0


if __name__ == '__main__':
    sys.exit(main())
