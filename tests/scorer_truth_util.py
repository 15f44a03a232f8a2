"""Shared rules of the fused-scorer tests against float64 (copied from tests/test_hip_scorer_f32.py:41-93 and the fp16 rule of
tests/test_hip_scorer2p.py:207, so that the tests of the wide lists (k = 33 .. 128) ask exactly what the k <= 32 tests ask).

Tolerance of one score: tol = C * 2^-24 * sum_d |u_d i_d|.
  * fp32-class route (``score_topk_f32s``): C = 64 — the three dropped partial products (<= 2^-23 |u_d i_d| each) and the fp32
    accumulation of the chain (6 D / 16 MFMAs into one accumulator), bounded with room.
  * fp16 route (``score_topk_f16``): truth is the float64 product of the fp16-ROUNDED operands (products of fp16 values are exact in
    fp32), so only the fp32 accumulation is left: C = D.
Two items whose float64 scores lie within 2 tol of each other may trade places in a list (near-ties); nothing else may. None of this
depends on the list length."""
import numpy as np
import scipy.sparse as sp
import torch

DEV = 'cuda'
C_TOL = 64.0


def S():
    import sibrar_amd
    return sibrar_amd


def excl(U, I_total, per, seed, heavy=()):
    """-> (host CSR, device CSR): `per` random exclusions per user, plus users with very long rows."""
    rng = np.random.default_rng(seed)
    rows, cols = [np.repeat(np.arange(U), per)], [rng.integers(0, I_total, size=U * per)]
    for (u, n) in heavy:
        rows.append(np.full(n, u))
        cols.append(rng.choice(I_total, size=n, replace=False))
    m = sp.csr_matrix((np.ones(sum(len(r) for r in rows), dtype=np.int8), (np.concatenate(rows), np.concatenate(cols))), shape=(U, I_total))
    m.sum_duplicates()
    m.sort_indices()
    return m, S().evaluation._csr_to_device(m, DEV)


def csr_of(rows, cols, shape):
    m = sp.csr_matrix((np.ones(sum(len(r) for r in rows), dtype=np.int8), (np.concatenate(rows), np.concatenate(cols))), shape=shape)
    m.sum_duplicates()
    m.sort_indices()
    return m, S().evaluation._csr_to_device(m, DEV)


def operands(route, u32, i32):
    """the representations as the route's arithmetic sees them (fp16 route: rounded to fp16, held in fp32) and the route's C"""
    if route == 'f16':
        return u32.half().float(), i32.half().float(), float(u32.shape[1])
    return u32, i32, C_TOL


def fused(route, u32, i32, k, users=None, ex=None, off=0):
    ops = S().ops
    if route == 'f16':
        fn, u_op, i_op = ops.score_topk_f16, u32.half(), i32.half()
    else:
        fn, u_op, i_op = ops.score_topk_f32s, u32, ops.split_bf16x3(i32)
    out = fn(u_op, i_op, k, item_offset=off) if ex is None else fn(u_op, i_op, k, users, ex[0], ex[1], item_offset=off)
    torch.cuda.synchronize()
    return out


def truth(u32, i32, rows, m=None, off=0, c=C_TOL):
    """float64 scores of the sampled users (excluded items -inf) and their tolerances"""
    u = u32[rows].double()
    s = u @ i32.double().t()
    tol = c * 2.0 ** -24 * (u.abs() @ i32.double().abs().t())
    if m is not None:
        dense = torch.from_numpy(m[rows.cpu().numpy()][:, off:off + i32.shape[0]].toarray() != 0).to(DEV)
        s[dense] = -float('inf')
    return s, tol


def check_against_truth(got, rows, s, tol, k, off=0, what=''):
    """every listed score within tol of its float64 score, no excluded or duplicated item, the float64 top-k up to near-ties, and
    (-inf, -1) behind the scoreable items of a user that has fewer than k"""
    val, idx = got[0][rows].double(), got[1][rows].long()
    assert val.shape[1] == k and idx.shape[1] == k
    n_ok = (s > -float('inf')).sum(1).clamp(max=k)
    valid = torch.arange(k, device=DEV)[None, :] < n_ok[:, None]
    assert bool(((idx >= 0) == valid).all()), f'{what}: list lengths differ from the scoreable item counts'
    assert bool((idx[~valid] == -1).all()) and bool((val[~valid] == -float('inf')).all()), f'{what}: padding is not (-inf, -1)'
    col = (idx - off).clamp(0, s.shape[1] - 1)
    assert bool(((idx - off)[valid] < s.shape[1]).all()) and bool(((idx - off)[valid] >= 0).all()), f'{what}: index outside the shard'
    s_pick, t_pick = s.gather(1, col), tol.gather(1, col)
    assert bool((s_pick[valid] > -float('inf')).all()), f'{what}: an excluded item was listed'
    err = (val - s_pick).abs()
    assert bool((err[valid] <= t_pick[valid]).all()), f'{what}: score error {float((err - t_pick)[valid].max())} over tol'
    srt = idx.sort(1).values
    assert not bool(((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)).any()), f'{what}: an item listed twice'
    kk = min(k, s.shape[1])
    tv, ti = torch.topk(s, kk, dim=1)
    t_truth = tol.gather(1, ti)
    gap = (s_pick[:, :kk] - tv).abs()
    ok = gap <= 2 * torch.maximum(t_pick[:, :kk], t_truth)
    assert bool(ok[valid[:, :kk]].all()), f'{what}: a list differs from the float64 top-k beyond near-ties (worst {float(gap[valid[:, :kk]].max())})'
    # scores descending, ties by item index ascending
    v, i = got[0][rows], got[1][rows]
    assert bool((v[:, :-1] >= v[:, 1:]).all()), f'{what}: scores not descending'
    tie = (v[:, :-1] == v[:, 1:]) & (i[:, 1:] >= 0)
    assert bool((i[:, :-1][tie] < i[:, 1:][tie]).all()), f'{what}: ties not by ascending item position'


def sample_rows(U):
    return torch.cat([torch.arange(min(U, 512)), torch.tensor([5, U - 1])]).unique().to(DEV)


def reps(U, I, D, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(U, D, generator=g) / 8).to(DEV), (torch.randn(I, D, generator=g) / 8).to(DEV)
