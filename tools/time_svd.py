"""SVD block iterations on synthetic 0/1 data at ML-1M's shape (6,040 users x 3,706 items, 946,068 interactions) and at 100,000 x 25,000
with 5,000,000 interactions, factors 64 and 100 (blocks of 92 and 128 columns): the time of one iteration of ``SVDAlgorithm.fit`` (two
sparse products, two Gram matrices, two eigen-decompositions, three rotations, the residual; device-event times, one warm-up, then the
median of --reps runs), of each kernel alone, and of a whole ``fit``; beside them ``torch.svd_lowrank`` on the same device (q = the same
block width, niter = the iterations the fit ran) as the composition to compare with. Prints one JSON line. Stand-alone: nothing is gated
on these figures.

    python tools/time_svd.py [--reps 3] [--small]
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sibrar_amd as S                                                            # noqa: E402
from time_als import synthetic, timed                                             # noqa: E402


def run(n_users, n_items, nnz, f, reps, dev):
    inter = synthetic(n_users, n_items, nnz)
    ops = S.ops
    x = S.features.DeviceCSR(inter).to(dev)
    t_indptr, t_indices, t_data = x.transposed()
    xt = SimpleNamespace(shape=(n_items, n_users), indptr=t_indptr, indices=t_indices, data=t_data)
    m = S.SVDAlgorithm(f, device=dev)
    b = min(f + m.oversample, n_users, n_items)
    orth = m._orth
    V, _, _ = orth(torch.from_numpy(m.initial_block(n_items, b)).to(dev))
    U, _, _ = orth(ops.csr_times_dense(x, V))                                      # one iteration in: a graded Gram matrix, as in every later one
    V, s, W = orth(ops.csr_times_dense(xt, U))
    Y = ops.csr_times_dense(x, V)
    G = ops.gram(Y)
    lam, Wy = ops.sym_eig(G)
    G0 = ops.gram(torch.from_numpy(m.initial_block(n_items, b)).to(dev))            # the first decomposition: a full matrix
    out = torch.empty_like(Y)

    def iteration():
        Yi = ops.csr_times_dense(x, V)
        ops.col_residual(Yi, U, s, f).max().item()
        Ui, _, _ = orth(Yi)
        _, _, Wi = orth(ops.csr_times_dense(xt, Ui))
        ops.rotate_cols(Ui, Wi, out=Ui)

    res = {'n_users': n_users, 'n_items': n_items, 'nnz': int(inter.nnz), 'factors': f, 'block': b,
           'iteration_ms': timed(iteration, reps),
           'x_times_v_ms': timed(lambda: ops.csr_times_dense(x, V, out=out), reps),
           'xt_times_u_ms': timed(lambda: ops.csr_times_dense(xt, U), reps),
           'gram_users_ms': timed(lambda: ops.gram(Y), reps),
           'sym_eig_graded_ms': timed(lambda: ops.sym_eig(G), reps),
           'sym_eig_full_ms': timed(lambda: ops.sym_eig(G0), reps),
           'rotate_users_ms': timed(lambda: ops.rotate_cols(Y, Wy, lam, out=out), reps),
           'residual_ms': timed(lambda: ops.col_residual(Y, U, s, f), reps)}
    fitted = S.SVDAlgorithm(f, device=dev).fit(inter)
    res['fit_iterations'] = fitted.n_iterations_run
    res['fit_residual_over_s0'] = fitted.residual / float(fitted.singular_values[0])
    res['fit_ms'] = timed(lambda: S.SVDAlgorithm(f, device=dev).fit(inter), reps)
    try:
        dense = torch.sparse_csr_tensor(x.indptr, x.indices.long(), torch.ones(x.indices.numel(), device=dev), size=(n_users, n_items))
        res['torch_svd_lowrank_ms'] = timed(lambda: torch.svd_lowrank(dense, q=b, niter=max(fitted.n_iterations_run, 1)), reps)
        sv = torch.svd_lowrank(dense, q=b, niter=max(fitted.n_iterations_run, 1))[1][:f]
        res['max_singular_value_diff_to_torch'] = float((sv - fitted.singular_values).abs().max() / sv[0])
    except Exception as e:                                                       # the composition is a comparison only
        res['torch_svd_lowrank_ms'] = None
        res['torch_error'] = f'{type(e).__name__}: {e}'[:200]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--small', action='store_true', help="ML-1M's shape only")
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    shapes = [(6040, 3706, 946068)] + ([] if args.small else [(100000, 25000, 5000000)])
    runs = [run(n, m, nnz, f, args.reps, dev) for n, m, nnz in shapes for f in (64, 100)]
    print(json.dumps({'bench': 'svd', 'reps': args.reps, 'device': torch.cuda.get_device_name(0), 'runs': runs}))


if __name__ == '__main__':
    main()
