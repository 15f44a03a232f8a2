"""Float64 references and derived bounds of the row-addressed table kernels (csrc/rowops.hip), evaluated on compact host copies of the
operands: what tests/test_hip_rowops.py states inline per case, as functions, for the modules that run the same entries on other
layouts (tests/test_hip_big_ld_rows.py). u = 2^-24 (hip_testutil.U32); an fp32 sum of m terms in any order errs by at most
m u sum|terms|. A plain module: no fixtures, no pytest hooks, no GPU."""
import numpy as np
import torch

from hip_testutil import U32


def _long(idx, n):
    return torch.arange(n) if idx is None else torch.as_tensor(np.asarray(idx), dtype=torch.long)


def scatter_add_ref(g, in_idx, rows, n_table, base=0.0):
    """dW[rows[j], :] = base + sum_j g[ii(j), :] -> (ref, bound, sources per table row [n_table, 1]). m atomic (or sorted) additions
    onto the existing value: (m + 1) u (|base| + sum|terms|); onto a zeroed table the first lands exactly: m u sum|terms|"""
    rt = _long(rows, len(rows))
    src = g[_long(in_idx, len(rt))].double()
    D = g.shape[1]
    ref = torch.full((n_table, D), float(base), dtype=torch.float64).index_add_(0, rt, src)
    mag = torch.full((n_table, D), abs(float(base)), dtype=torch.float64).index_add_(0, rt, src.abs())
    m = torch.bincount(rt, minlength=n_table).double()[:, None]
    return ref, (m if base == 0.0 else m + 1) * U32 * mag, m


def bag_mean_fwd_ref(W, tags, pad, rows):
    """out[j] = mean over the non-pad tags of entity rows[j] -> (ref, bound, cnt): (cnt + 1) u sum|terms| / cnt"""
    tg = torch.as_tensor(np.asarray(tags))[_long(rows, len(rows))]
    live = tg != pad
    cnt = live.sum(1)
    terms = W.double()[tg] * live[:, :, None]
    den = cnt.clamp_min(1).double()[:, None]
    return terms.sum(1) / den, (cnt + 1).double()[:, None] * U32 * terms.abs().sum(1) / den, cnt


def bag_mean_bwd_ref(g, in_idx, tags, pad, rows, n_tags):
    """dW[tag] += g[ii(j)] / cnt_j for every live tag of slot j -> (ref, bound, m [n_tags, 1]): (m + 1) u sum|terms|"""
    tg = torch.as_tensor(np.asarray(tags))[_long(rows, len(rows))]
    live = tg != pad
    den = live.sum(1).clamp_min(1).double()[:, None]
    D = g.shape[1]
    contrib = (g[_long(in_idx, len(tg))].double()[:, None, :] / den[:, :, None]) * live[:, :, None]
    flat = tg.reshape(-1)
    ref = torch.zeros(n_tags, D, dtype=torch.float64).index_add_(0, flat, contrib.reshape(-1, D))
    mag = torch.zeros(n_tags, D, dtype=torch.float64).index_add_(0, flat, contrib.reshape(-1, D).abs())
    m = torch.zeros(n_tags, dtype=torch.float64).index_add_(0, flat, live.reshape(-1).double())[:, None]
    return ref, (m + 1) * U32 * mag, m


def csr_dense(indptr, indices, vals, n_rows, n_cols):
    """the CSR matrix as float64 [n_rows, n_cols]; vals None: ones"""
    d = torch.zeros(n_rows, n_cols, dtype=torch.float64)
    for r in range(n_rows):
        lo, hi = int(indptr[r]), int(indptr[r + 1])
        d[r, torch.as_tensor(np.asarray(indices[lo:hi]), dtype=torch.long)] = 1.0 if vals is None else torch.as_tensor(np.asarray(vals[lo:hi])).double()
    return d


def csr_project_fwd_ref(dense, rows, wt, bias):
    """out[j] = bias + dense[rows[j]] @ Wt (act none) -> (ref, bound): a row of q nnz, (q + 1) u sum|terms|"""
    d = dense[_long(rows, len(rows))]
    q = (d != 0).sum(1, keepdim=True).double()
    b = torch.zeros(wt.shape[1], dtype=torch.float64) if bias is None else bias.double()
    return d @ wt.double() + b, (q + 1) * U32 * (d.abs() @ wt.double().abs() + b.abs())


def csr_project_bwd_ref(dense, rows, dz, dz_idx=None, base=0.0, extra=1):
    """dWt = base + dense[rows]^T dZ[di(j)] -> (ref, bound): m sources per column, (m + extra) u (|base| + sum|terms|); extra = 1 for the
    scatter form, 2 for the gather form"""
    d = dense[_long(rows, len(rows))]
    z = dz[_long(dz_idx, len(d))].double()
    m = (d != 0).sum(0).double()[:, None]
    return d.t() @ z + base, (m + extra) * U32 * (d.abs().t() @ z.abs() + abs(base))
