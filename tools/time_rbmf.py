"""RBMF.fit on synthetic 0/1 data at ML-1M's shape (6,040 users x 3,706 items, 946,068 interactions) and at 100,000 x 25,000 with
5,000,000 interactions, 64 and 128 representatives, split by phase: the SVD's block iteration (capped at --svd-iterations), the LU
chain (r launches of sbr_maxvol_lu_step_f32 and B = L L_top^-1), the swap chain (the whole of ``ops.maxvol`` less the LU chain) and the
ridge solve (the gather of C, the Gram matrix, the sparse product, the Cholesky factor, two triangular solves); device-event times, one
warm-up, then the median of --reps runs. Beside them a composition of torch's own operators on the same device and the same U:
``torch.linalg.lu`` of U for the pivots, ``torch.linalg.solve`` for B, the dense rank-1 update loop with ``argmax``, and
``torch.linalg.solve`` for the ridge system. Prints one JSON line. Stand-alone: nothing is gated on these figures.

    python tools/time_rbmf.py [--reps 3] [--small] [--svd-iterations 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sibrar_amd as S                                                            # noqa: E402
from time_als import synthetic, timed                                             # noqa: E402


def torch_maxvol(U, tol, max_iters):
    """the same algorithm from torch's operators -> (idx, swaps, ms of the LU start, ms of the swap loop)"""
    r = U.shape[1]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    _, pivots = torch.linalg.lu_factor(U)
    perm = torch.arange(U.shape[0], device=U.device)
    for k, p in enumerate((pivots[:r] - 1).tolist()):                            # LAPACK's row interchanges -> the pivot rows
        perm[[k, p]] = perm[[p, k]]
    idx = perm[:r].clone()
    B = torch.linalg.solve(U[idx].t(), U.t()).t().contiguous()
    ev[1].record()
    swaps = 0
    while swaps < max_iters:
        flat = int(B.abs().argmax())
        i, j = divmod(flat, r)
        if not abs(float(B[i, j])) > tol:
            break
        w = B[i].clone()
        w[j] -= 1
        B -= torch.outer(B[:, j].clone(), w / B[i, j])
        idx[j] = i
        swaps += 1
    ev[2].record()
    torch.cuda.synchronize()
    return idx, swaps, ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])


def run(n_users, n_items, nnz, r, reps, svd_iterations, dev):
    inter = synthetic(n_users, n_items, nnz)
    ops = S.ops
    x = S.features.DeviceCSR(inter).to(dev)
    m = S.RBMF(r, device=dev, n_iterations=svd_iterations)
    b = min(r + m.oversample, n_users, n_items)
    v0 = m.initial_block(n_items, b)
    svd = sys.modules[S.SVDAlgorithm.__module__]
    U = svd.block_iteration(inter, v0, r, svd_iterations, m.svd_tol, dev, x=x)[0][:, :r].contiguous()

    def lu_chain():
        B = U.clone()
        _, ltop, _ = ops.maxvol_lu(B)
        return ops.tri_solve_rows(B, ltop, unit=True, out=B)

    def ridge(idx):
        Ct = torch.from_numpy(np.ascontiguousarray(inter[idx.cpu().numpy()].toarray().T, dtype=np.float32)).to(dev)
        M = ops.csr_times_dense(x, Ct)
        R = ops.cholesky(ops.als_gram(Ct, float(m.lam)))
        return ops.tri_solve_rows(ops.tri_solve_rows(M, R.t().contiguous(), upper=True, out=M), R, out=M), Ct

    def torch_ridge(idx):
        Ct = torch.from_numpy(np.ascontiguousarray(inter[idx.cpu().numpy()].toarray().T, dtype=np.float32)).to(dev)
        dense = torch.sparse_csr_tensor(x.indptr, x.indices.long(), torch.ones(x.indices.numel(), device=dev), size=(n_users, n_items))
        K = Ct.t() @ Ct + float(m.lam) * torch.eye(r, device=dev)
        return torch.linalg.solve(K, (dense @ Ct).t()).t()

    idx, swaps = ops.maxvol(U, m.tol, m.max_iters)
    res = {'n_users': n_users, 'n_items': n_items, 'nnz': int(inter.nnz), 'r': r, 'svd_iterations': svd_iterations, 'swaps': swaps,
           'svd_ms': timed(lambda: svd.block_iteration(inter, v0, r, svd_iterations, m.svd_tol, dev, x=x), reps),
           'lu_chain_ms': timed(lu_chain, reps),
           'maxvol_ms': timed(lambda: ops.maxvol(U, m.tol, m.max_iters), reps),
           'ridge_ms': timed(lambda: ridge(idx), reps),
           'fit_ms': timed(lambda: S.RBMF(r, device=dev, n_iterations=svd_iterations).fit(inter), reps)}
    res['swap_chain_ms'] = res['maxvol_ms'] - res['lu_chain_ms']
    try:
        runs = [torch_maxvol(U, m.tol, m.max_iters) for _ in range(reps + 1)][1:]
        res['torch_lu_ms'], res['torch_swap_loop_ms'] = float(np.median([t[2] for t in runs])), float(np.median([t[3] for t in runs]))
        res['torch_swaps'], res['torch_same_set'] = runs[0][1], set(runs[0][0].tolist()) == set(idx.tolist())
        res['torch_ridge_ms'] = timed(lambda: torch_ridge(idx), reps)
        res['max_x_diff_to_torch'] = float((torch_ridge(idx) - ridge(idx)[0]).abs().max())
    except Exception as e:                                                       # the composition is a comparison only
        res['torch_error'] = f'{type(e).__name__}: {e}'[:200]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--small', action='store_true', help="ML-1M's shape only")
    ap.add_argument('--svd-iterations', type=int, default=10)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    shapes = [(6040, 3706, 946068)] + ([] if args.small else [(100000, 25000, 5000000)])
    runs = [run(n, m, nnz, r, args.reps, args.svd_iterations, dev) for n, m, nnz in shapes for r in (64, 128)]
    print(json.dumps({'bench': 'rbmf', 'reps': args.reps, 'device': torch.cuda.get_device_name(0), 'runs': runs}))


if __name__ == '__main__':
    main()
