"""Times NGCF's fused layer on the GPU on the ML-1M-shaped synthetic world (6,040 x 3,706, 1,000,209 interactions) at
D = 64 with three layers: the forward stack (``ops.NGCFPropagateFn``, three ``sbr_ngcf_layer_fwd`` launches) and forward + backward,
beside the composition of existing pieces on the same inputs (``ops.graph_propagate``, torch elementwise ops, ``torch.matmul``,
``F.leaky_relu``, ``F.dropout``, ``F.normalize``, with torch autograd and ``ops.graph_propagate`` as its own backward); the gather alone
(``ops.graph_propagate``) and the two products alone (``torch.matmul``), to say which of them dominates; and one training step at batch
8,192 of ``ngcf`` beside ``lightgcn``. Every GPU step runs in a child process under its own time limit; the first step that fails or
runs out of time is reported (``stopped`` names it), no further step is started and the exit status is 1. Device events around
``--launches`` calls after a warm-up, the median of ``--reps``. Prints one JSON line; times in milliseconds per call.

    python tools/time_ngcf.py [--reps 5] [--launches 50] [--limit 240]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = 'cuda'
USERS, ITEMS, NNZ, D, LAYERS, P, SLOPE = 6040, 3706, 1000209, 64, 3, 0.1, 0.2


def timed(fn, reps, launches):
    import torch
    fn()                                                          # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / launches)
    return statistics.median(out)


def _world():
    import torch
    import sibrar_amd as S
    S.reproducible(0, deterministic=False)
    ds = S.SyntheticDataset(USERS, ITEMS, NNZ, seed=0, n_negative_samples=4)
    return S, ds, torch


def step_layers(reps, launches):
    S, ds, torch = _world()
    import torch.nn.functional as F
    ops = S.ops
    net = S.NGCF(USERS, ITEMS, ds.user_sampling_matrix_train, D, (D,) * LAYERS, P, SLOPE).to(DEV)
    csr = net._graph
    e0 = torch.cat([net.user_embeddings.weight, net.item_embeddings.weight]).detach().mul(64).requires_grad_()
    params = [t.detach().clone().requires_grad_() for t in net._layer_params()]
    g_table = torch.randn(USERS + ITEMS, D * (LAYERS + 1), device=DEV)

    class Prop(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return ops.graph_propagate(csr, x)

        @staticmethod
        def backward(ctx, g):
            return ops.graph_propagate(csr, g.contiguous())

    def fused(backward):
        t = ops.NGCFPropagateFn.apply(csr, e0, SLOPE, P, 1, *params)
        if backward:
            torch.autograd.grad(t, [e0] + params, g_table)
        return t

    def composed(backward):
        x, parts = e0, [e0]
        for l in range(LAYERS):
            W1, W2, b = params[3 * l:3 * l + 3]
            s = Prop.apply(x)
            x = F.dropout(F.leaky_relu(torch.matmul(s + x, W1) + torch.matmul(s * x, W2) + b, SLOPE), P, True)
            parts.append(F.normalize(x, dim=1))
        t = torch.cat(parts, 1)
        if backward:
            torch.autograd.grad(t, [e0] + params, g_table)
        return t

    with torch.no_grad():
        diff = float((ops.NGCFPropagateFn.apply(csr, e0, SLOPE, 0.0, 1, *params) - _no_dropout(composed, F)).abs().max())
        x = e0.detach()
        y = torch.empty_like(x)
        res = {'gather_ms': timed(lambda: ops.graph_propagate(csr, x, out=y), reps, launches),
               'two_products_ms': timed(lambda: torch.matmul(x, params[0]) + torch.matmul(y, params[1]), reps, launches),
               'fused_fwd_ms': timed(lambda: fused(False), reps, launches), 'composed_fwd_ms': timed(lambda: composed(False), reps, launches)}
    res.update({'fused_fwd_bwd_ms': timed(lambda: fused(True), reps, launches), 'composed_fwd_bwd_ms': timed(lambda: composed(True), reps, launches),
                'max_abs_difference_without_dropout': diff, 'rows': USERS + ITEMS, 'D': D, 'layers': LAYERS})
    return res


def _no_dropout(composed, F):
    """the composition with the dropout switched off, for the comparison of values"""
    keep, F.dropout = F.dropout, (lambda x, p, training: x)
    try:
        return composed(False)
    finally:
        F.dropout = keep


def step_train(which, reps, launches):
    S, ds, torch = _world()
    conf = {'embedding_dim': D, 'layer_sizes': (D,) * LAYERS, 'n_layers': LAYERS, 'message_dropout': P}
    net = S.ALGORITHMS[which].build_from_conf(conf, ds)
    loss = S.RecBayesianPersonalizedRankingLoss(n_items=ITEMS, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=4)
    tr = S.Trainer(net, None, None, loss, {'learn': {'lr': 1e-3, 'wd': 1e-5, 'optimizer': 'adamw'}, 'run_settings': {'device': DEV}})
    net.train()
    batch = next(iter(S.NegativeSamplingDataLoader(ds, batch_size=8192, shuffle=True)))
    return {'train_step_ms': timed(lambda: tr.train_step(*batch), reps, max(1, launches // 5))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--limit', type=int, default=240, help='seconds a child may run')
    ap.add_argument('--step', default=None, help='(internal) run one step in this process')
    args = ap.parse_args()
    if args.step is not None:
        kind, *rest = args.step.split(':')
        res = step_layers(args.reps, args.launches) if kind == 'layers' else step_train(rest[0], args.reps, args.launches)
        print('RESULT ' + json.dumps(res))
        return
    runs = {'reps': args.reps, 'launches': args.launches}
    for step in ('layers', 'train:ngcf', 'train:lightgcn'):
        cmd = [sys.executable, os.path.abspath(__file__), '--step', step, '--reps', str(args.reps), '--launches', str(args.launches)]
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
    print(json.dumps({'bench': 'ngcf', **runs}))
    if 'stopped' in runs:
        sys.exit(1)


if __name__ == '__main__':
    main()
