"""ALS half-sweeps on synthetic 0/1 data at ML-1M's shape (6,040 users x 3,706 items, 946,068 interactions) and at 100,000 x 25,000
with 5,000,000 interactions, factors 64 and 128: the time of a user and of an item half-sweep (ops.als_gram + ops.als_solve_rows,
device-event times, one warm-up, then the median of --reps runs), and beside each the time of a torch composition of the same update on
the same device — a padded gather of the rows' y_i per user chunk, torch.bmm for the chunk's A_r, torch.linalg.cholesky and
torch.cholesky_solve. Prints one JSON line. Stand-alone: nothing is gated on these figures.

    python tools/time_als.py [--reps 3] [--small]
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sibrar_amd as S                                                            # noqa: E402

ALPHA, REG = 40.0, 0.01
GATHER_BYTES = 1 << 29                 # at most 512 MiB of gathered rows per chunk of the composition


def synthetic(n_users, n_items, nnz, seed=0):
    """log-normal user degrees, uniform items, 0/1"""
    rng = np.random.default_rng(seed)
    deg = rng.lognormal(0., 1., n_users)
    deg = np.clip(np.round(deg * nnz / deg.sum()), 1, n_items).astype(np.int64)
    rows = np.repeat(np.arange(n_users), deg)
    cols = rng.integers(0, n_items, size=rows.size)
    m = sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(n_users, n_items))
    m.sum_duplicates()
    m.data[:] = 1
    m.sort_indices()
    return m


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def torch_half_sweep(csr, Y):
    """the same update from torch's own operators, one user chunk at a time"""
    n, f = csr.shape[0], Y.shape[1]
    G = Y.t() @ Y + REG * torch.eye(f, device=Y.device)
    counts = csr.indptr[1:] - csr.indptr[:-1]
    out = torch.zeros(n, f, device=Y.device)
    longest = max(int(counts.max()), 1)
    step = max(1, min(n, GATHER_BYTES // (4 * f * longest)))
    ar = torch.arange(longest, device=Y.device)
    for lo in range(0, n, step):
        hi = min(lo + step, n)
        cnt = counts[lo:hi]
        L = max(int(cnt.max()), 1)
        valid = ar[None, :L] < cnt[:, None]
        pos = (csr.indptr[lo:hi, None] + ar[None, :L]).clamp_(max=csr.indices.numel() - 1)
        Yp = Y[csr.indices[pos].long()] * valid[:, :, None]                       # [B, L, f], zero rows behind a user's entries
        A = G[None] + torch.bmm(Yp.transpose(1, 2) * (ALPHA - 1.), Yp)
        b = ALPHA * Yp.sum(dim=1)
        out[lo:hi] = torch.cholesky_solve(b[:, :, None], torch.linalg.cholesky(A))[:, :, 0]
    return out * (counts > 0)[:, None]


def run(n_users, n_items, nnz, f, reps, dev):
    inter = synthetic(n_users, n_items, nnz)
    x = S.features.DeviceCSR(inter).to(dev)
    t_indptr, t_indices, t_data = x.transposed()
    xt = SimpleNamespace(shape=(n_items, n_users), indptr=t_indptr, indices=t_indices, data=t_data)
    m = S.AlternatingLeastSquare(ALPHA, f, REG, 1, device=dev)
    u0, i0 = (torch.from_numpy(a).to(dev) for a in m.initial_factors(n_users, n_items))
    users = S.ops.als_solve_rows(x, i0, S.ops.als_gram(i0, REG), ALPHA)            # one half-sweep in: factors of a realistic scale
    res = {'n_users': n_users, 'n_items': n_items, 'nnz': int(inter.nnz), 'factors': f}
    for side, csr, Y in (('user', x, i0), ('item', xt, users)):
        res[f'{side}_gram_ms'] = timed(lambda: S.ops.als_gram(Y, REG), reps)
        G = S.ops.als_gram(Y, REG)
        out = torch.empty(csr.shape[0], f, device=dev)
        res[f'{side}_half_sweep_ms'] = timed(lambda: S.ops.als_solve_rows(csr, Y, S.ops.als_gram(Y, REG), ALPHA, out=out), reps)
        try:
            res[f'{side}_torch_ms'] = timed(lambda: torch_half_sweep(csr, Y), reps)
            ref = torch_half_sweep(csr, Y)
            res[f'{side}_max_diff_to_torch'] = float((ref - S.ops.als_solve_rows(csr, Y, G, ALPHA)).abs().max() / ref.abs().max())
        except Exception as e:                                                   # the composition is a comparison only
            res[f'{side}_torch_ms'] = None
            res[f'{side}_torch_error'] = f'{type(e).__name__}: {e}'[:200]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--small', action='store_true', help="ML-1M's shape only")
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    shapes = [(6040, 3706, 946068)] + ([] if args.small else [(100000, 25000, 5000000)])
    runs = [run(n, m, nnz, f, args.reps, dev) for n, m, nnz in shapes for f in (64, 128)]
    print(json.dumps({'bench': 'als', 'alpha': ALPHA, 'regularization': REG, 'reps': args.reps, 'device': torch.cuda.get_device_name(0),
                      'runs': runs}))


if __name__ == '__main__':
    main()
