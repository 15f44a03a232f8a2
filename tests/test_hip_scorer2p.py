"""GPU: the two-pass fused scorer (csrc/score_topk_f16_2p.hip: group-maxima pass, pair selection, grouped re-scoring, final selection)
against the one-pass kernel (csrc/score_topk_f16_n.hip, itself pinned against the fp32 GEMM + exact top-k route and through it against
eval/eval.py:216-222) — the two routes must return the SAME lists bit for bit (same MFMA chain per score, same ordering rule: score
desc, item index asc) — and directly against the fp32 route on samples."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def S():
    import sibrar_amd
    return sibrar_amd


def _excl(U, I_total, per, seed, heavy=()):
    rng = np.random.default_rng(seed)
    rows, cols = [np.repeat(np.arange(U), per)], [rng.integers(0, I_total, size=U * per)]
    for (u, n) in heavy:                                       # users with very long exclusion rows
        rows.append(np.full(n, u))
        cols.append(rng.choice(I_total, size=n, replace=False))
    m = sp.csr_matrix((np.ones(sum(len(r) for r in rows), dtype=np.int8), (np.concatenate(rows), np.concatenate(cols))), shape=(U, I_total))
    m.sum_duplicates()
    m.sort_indices()
    return S().evaluation._csr_to_device(m, DEV)


def _both(u16, i16, k, users=None, ex=None, off=0):
    ops = S().ops
    out = []
    for route in (1, 2):
        prev = ops.score_topk_route(route)
        try:
            if ex is None:
                out.append(ops.score_topk_f16(u16, i16, k, item_offset=off))
            else:
                out.append(ops.score_topk_f16(u16, i16, k, users, ex[0], ex[1], item_offset=off))
        finally:
            ops.score_topk_route(prev)
    torch.cuda.synchronize()
    return out


def _same(a, b, what=''):
    (v1, i1), (v2, i2) = a, b
    bad = (i1 != i2).any(dim=1) | (v1 != v2).any(dim=1)
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} users differ, first {int(bad.nonzero()[0])}: one-pass {i1[bad][0].tolist()} two-pass {i2[bad][0].tolist()}'


TIGHT_CAP = 0.0005      # the fp32-class scorer's cap (test_hip_scorer_f32.py: >= 0.9995 of the positions identical)


def _near(got, ref, sc, off=0, cap=0.01):
    """Against the fp32 GEMM route: the same lists, except that two items whose fp32 scores differ by rounding only (the GEMM sums in
    another order than the MFMA chain) may trade places — every listed item's fp32 score is within 2e-6 of the reference list's score at
    that rank, and no excluded item is listed. At most ``cap`` of the positions may differ. Only a position whose item is within the
    2e-6 score clause of its neighbour in rank CAN legitimately differ, so a cap is justified where the float64 scores of the same
    fp16-rounded operands have fewer such positions than it allows. Counted on the CPU (float64 product, exclusions applied, the
    sampled users, ranks 0 .. k against their neighbours): 2 / 10,240 at (3000, 20000, 128), 4 / 10,240 at (40000, 30011, 128), 0 / 512 at
    (777, 8192, 128) and 7 / 15,000 for the user-index-map test — below TIGHT_CAP, which those callers pass; 6 / 5,120 at (2500, 16384, 64),
    6 / 10,240 at (1100, 9000, 256), 14 / 16,384 at (9000, 12345, 256) and 8 / 10,240 at (33000, 8700, 64) — above it, so those keep 1 %."""
    (gv, gi), (rv, ri) = got, ref
    n = rv.shape[0]
    picked = torch.gather(sc[:n], 1, (gi[:n].long() - off).clamp_min(0))
    assert bool((picked > -float('inf')).all()), 'an excluded item was listed'
    assert bool(((picked - rv).abs() <= 2e-6 * rv.abs().clamp_min(1.0)).all()), 'a listed item is not a top-k item of the fp32 route'
    frac = float((gi[:n].long() != ri.long() + off).float().mean())
    assert frac < cap, f'{frac:.5f} of the positions differ from the fp32 route (cap {cap})'


_TIGHT_SHAPES = {(3000, 20000, 128), (40000, 30011, 128), (777, 8192, 128)}


@pytest.mark.parametrize('U,I,D,k,per,off', [(3000, 20000, 128, 20, 30, 0), (2500, 16384, 64, 10, 0, 0), (1100, 9000, 256, 20, 25, 5000),
                                             (40000, 30011, 128, 20, 50, 0), (9000, 12345, 256, 32, 10, 777), (777, 8192, 128, 1, 5, 0),
                                             (33000, 8700, 64, 20, 40, 100)])
def test_two_pass_scorer_equals_the_one_pass_kernel(U, I, D, k, per, off):
    """Random representations, exclusions (per user `per` random items of the whole catalogue; the shard starts at `off`), catalogue
    sizes that end inside a supertile / a tile, user counts with remainder units and part waves, every supported D, k = 1 .. 32."""
    g = torch.Generator().manual_seed(U + I)
    u16 = (torch.randn(U, D, generator=g) / 8).half().to(DEV)
    i16 = (torch.randn(I, D, generator=g) / 8).half().to(DEV)
    users = torch.arange(U, device=DEV)
    ex = _excl(U, off + I + 100, per, U, heavy=((5, 3000), (U - 1, 6000))) if per else None
    one, two = _both(u16, i16, k, users, ex, off)
    _same(one, two, f'{U}x{I}x{D}')
    # and a sample directly against the fp32 GEMM -> mask -> exact top-k route
    n = min(U, 512)
    sc = u16[:n].float() @ i16.float().t()
    if ex is not None:
        S().ops.mask_scores_(sc, users[:n], ex[0], ex[1], item_offset=off)
    rv, ri = S().ops.topk_rows(sc, k)
    _near((two[0][:n], two[1][:n]), (rv, ri), sc, off, cap=TIGHT_CAP if (U, I, D) in _TIGHT_SHAPES else 0.01)


def test_two_pass_scorer_with_massive_ties_and_degenerate_users():
    """Hard users take the exact slow path of the final kernel: all-equal scores (every group ties at the bound), a user whose row is
    zero, users with fewer than k scoreable items (everything else excluded), duplicated items (exact ties between groups)."""
    g = torch.Generator().manual_seed(3)
    U, I, D, k = 600, 10000, 128, 20
    u16 = (torch.randn(U, D, generator=g) / 8).half()
    i16 = (torch.randn(I, D, generator=g) / 8).half()
    u16[7] = 0                                                   # every score 0: the first k items win
    i16[2000:6000] = i16[0:4000].clone()                                 # 4,000 exact duplicates: ties across groups and supertiles
    u16, i16 = u16.to(DEV), i16.to(DEV)
    rng = np.random.default_rng(1)
    rows, cols = [], []
    for u in range(U):
        if u == 11:                                              # 5 scoreable items only
            c = np.setdiff1d(np.arange(I), [3, 4000, 4001, 9998, 9999])
        elif u == 12:                                            # nothing scoreable
            c = np.arange(I)
        else:
            c = rng.integers(0, I, size=20)
        rows.append(np.full(len(c), u)); cols.append(c)
    m = sp.csr_matrix((np.ones(sum(len(r) for r in rows), dtype=np.int8), (np.concatenate(rows), np.concatenate(cols))), shape=(U, I))
    m.sum_duplicates(); m.sort_indices()
    ex = S().evaluation._csr_to_device(m, DEV)
    users = torch.arange(U, device=DEV)
    one, two = _both(u16, i16, k, users, ex)
    _same(one, two, 'ties')
    assert two[1][12].tolist() == [-1] * k and two[1][11, 5:].tolist() == [-1] * (k - 5)
    assert sorted(two[1][11, :5].tolist()) == [3, 4000, 4001, 9998, 9999]
    # constant catalogue: every user is hard
    i_const = i16[:1].expand(9000, D).contiguous()
    one, two = _both(u16[:100], i_const, k)
    _same(one, two, 'constant catalogue')
    assert two[1][0].tolist() == list(range(k))


def test_two_pass_scorer_at_the_bench_shapes():
    """BASELINE configs[1] / [4] scoring shapes (100k x 50k x 128 with ~50 exclusions per user; 100k x 25k x 256, shard offset 75,000)."""
    for (U, I, D, off) in ((100_000, 50_000, 128, 0), (100_000, 25_000, 256, 75_000)):
        g = torch.Generator().manual_seed(D)
        u16 = (torch.randn(U, D, generator=g) / 16).half().to(DEV)
        i16 = (torch.randn(I, D, generator=g) / 16).half().to(DEV)
        users = torch.arange(U, device=DEV)
        ex = _excl(U, off + I, 50, D, heavy=((17, 3345),))
        one, two = _both(u16, i16, 20, users, ex, off)
        _same(one, two, f'{U}x{I}x{D}')


def test_both_scorer_routes_with_a_user_index_map():
    """``u_idx`` maps the scored rows to rows of the exclusion CSR (an evaluation chunk of a split whose users are not 0 .. U - 1): both
    routes read the exclusions of the mapped user, and agree with the fp32 route."""
    g = torch.Generator().manual_seed(17)
    U, I, D, k = 1500, 9000, 128, 10
    n_all = 5000
    u16 = (torch.randn(U, D, generator=g) / 8).half().to(DEV)
    i16 = (torch.randn(I, D, generator=g) / 8).half().to(DEV)
    ex = _excl(n_all, I, 40, 17, heavy=((4321, 2500),))
    users = torch.randperm(n_all, generator=g)[:U].to(DEV)          # int64 user ids in scoring order
    users[7] = 4321
    one, two = _both(u16, i16, k, users, ex)
    _same(one, two, 'u_idx')
    sc = u16.float() @ i16.float().t()
    S().ops.mask_scores_(sc, users, ex[0], ex[1])
    rv, ri = S().ops.topk_rows(sc, k)
    _near(two, (rv, ri), sc, cap=TIGHT_CAP)


def _guarded_bytes(nbytes, pad=4096):
    """uint8 view of ``nbytes`` inside a buffer of 0xFF bytes (as fp32 / int32: NaN / -1)"""
    whole = torch.full((pad + max(nbytes, 16) + pad,), 0xFF, dtype=torch.uint8, device=DEV)
    return whole, whole[pad:pad + max(nbytes, 16)]


def _fused_guarded(entry, u, i_op, I, k, users, ex, guard=64):
    """One call of a fused scorer C entry whose user matrix ``u`` is the head of a larger allocation and whose outputs, workspace and
    event stream are views into larger pattern-filled buffers -> (val, idx) after asserting that every guard still holds its pattern."""
    mod = S()
    from importlib import import_module
    _lib = import_module(mod.ops.__name__.rsplit('.', 1)[0] + '._lib')
    lib, ptr = _lib.lib(), _lib.ptr
    Bu, D = u.shape
    val_all = torch.full((guard + Bu + guard, k), float('nan'), device=DEV)
    idx_all = torch.full((guard + Bu + guard, k), -777, dtype=torch.int32, device=DEV)
    val, idx = val_all[guard:guard + Bu], idx_all[guard:guard + Bu]
    ws_all, ws = _guarded_bytes(int(getattr(lib, entry + '_workspace')(Bu, I, k)))
    nnz = int(ex[1].numel())
    ev_all, ev = _guarded_bytes(int(lib.sbr_score_topk_f16_events_bytes(Bu, nnz)) + 16)
    _lib.call(entry, ptr(u), ptr(i_op), D, Bu, I, ptr(users), ptr(ex[0]), ptr(ex[1]), nnz, 0, k, ptr(val), ptr(idx), ptr(ws), ws.numel(),
              ptr(ev), ev.numel(), 1, mod.ops.stream())
    torch.cuda.synchronize()
    for name, whole, inner in (('workspace', ws_all, ws), ('event stream', ev_all, ev)):
        pad = (whole.numel() - inner.numel()) // 2
        assert bool((whole[:pad] == 0xFF).all()) and bool((whole[pad + inner.numel():] == 0xFF).all()), f'{entry}: wrote outside its {name}'
    assert bool(torch.isnan(val_all[:guard]).all()) and bool(torch.isnan(val_all[guard + Bu:]).all()), f'{entry}: wrote value rows of users >= Bu'
    assert bool((idx_all[:guard] == -777).all()) and bool((idx_all[guard + Bu:] == -777).all()), f'{entry}: wrote index rows of users >= Bu'
    return val.clone(), idx.clone()


def test_non_finite_scores_with_a_ragged_user_count_on_all_three_fused_routes():
    """+inf scores with Bu % 32 != 0 (the select ballot and the rescore append of the two-pass scorer compare against L = +inf for lanes
    without a user, which a +inf score passes: validity is gated by index). 1,013 users x 9,000 items x 128, k = 10, exclusions on.
    Item 1234 gets +inf in column 3 through the overflow of the fp16 cast (fp32 1e6), item 5678 an explicit +inf in column 77, item 8000
    an explicit -inf in column 5, item 4321 finite values of 6e4 (scores of ~1e5, far outside the fp16 range). The scorers accumulate and
    return fp32 scores, so fp16 overflow enters through the OPERANDS only: the reference is the float64 product of the fp16-rounded
    operands, in which an infinite operand makes the score +-inf by the sign of the user's entry in that column (no user entry there is
    zero, asserted: no NaN score in this test). Items with score +inf lead the lists in index order; items with score -inf are never
    listed (9,000 items outrank them). The user matrix is the head of an allocation with 64 more rows of large finite values; outputs,
    workspace and event stream are views into pattern-filled buffers, so a lane that reads or writes a row >= Bu stays inside memory of
    this test and shows as a wrong list or a disturbed guard. fp16 one-pass == fp16 two-pass bit for bit, both == the reference up to
    fp32 rounding (tol = D 2^-24 sum|u_d i_d| per score; near-ties within 2 tol may trade places).
    The fp32-class route on the same values with finite items agrees with float64 truth (_check_against_truth of test_hip_scorer_f32.py).
    With the +inf column its item split gives the planes (inf, NaN, NaN) — inf - inf — hence NaN scores: non-finite item values are not
    supported by 'fp32_fused'; ``ops.split_bf16x3_supported`` reports it and the evaluator falls back to the 'fp32' route. The scorer is
    still launched once on those planes: it must stay inside its buffers (what it lists is recorded in the message, not asserted)."""
    ops = S().ops
    U, I, D, k, G = 1013, 9000, 128, 10, 64
    g = torch.Generator().manual_seed(99)
    u_all = (torch.randn(U + G, D, generator=g) / 8).half()
    u_all[u_all == 0] = 0.01
    u_all[U:] = 100.0                                            # guard rows: would win every list if scored
    i32 = (torch.randn(I, D, generator=g) / 8).half().float()
    i32[4321] = 60000.0 * torch.sign(torch.randn(D, generator=g))
    i32[1234, 3] = 1e6
    i16 = ops.cast_f16(i32.to(DEV))
    assert float(i16[1234, 3]) == float('inf')
    i16[5678, 77] = float('inf')
    i16[8000, 5] = -float('inf')
    u_all_d = u_all.to(DEV)
    u16 = u_all_d[:U]
    assert u16.data_ptr() == u_all_d.data_ptr() and bool((u16[:, [3, 77, 5]] != 0).all())
    users = torch.arange(U, device=DEV)
    rng = np.random.default_rng(5)
    rows = np.concatenate([np.repeat(np.arange(U), 20), np.arange(0, U, 7), np.arange(3, U, 11)])
    cols = np.concatenate([rng.integers(0, I, size=U * 20), np.full(len(np.arange(0, U, 7)), 1234), np.full(len(np.arange(3, U, 11)), 5678)])
    m = sp.csr_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(U, I))
    m.sum_duplicates(); m.sort_indices()
    ex = S().evaluation._csr_to_device(m, DEV)
    out = {}
    for route in (1, 2):
        prev = ops.score_topk_route(route)
        try:
            out[route] = _fused_guarded('sbr_score_topk_f16', u16, i16, I, k, users, ex, G)
        finally:
            ops.score_topk_route(prev)
    _same(out[1], out[2], 'non-finite scores')
    # float64 reference of the fp16-rounded operands (CPU)
    uh, ih = u16.cpu().double(), i16.cpu().double()
    with np.errstate(all='ignore'):
        s = uh @ torch.nan_to_num(ih, posinf=0.0, neginf=0.0).t()
        for (it, c) in ((1234, 3), (5678, 77), (8000, 5)):
            s[:, it] = uh[:, c] * ih[it, c]                      # +-inf by the sign of the user's entry
    assert not bool(torch.isnan(s).any())
    tol = D * 2.0 ** -24 * (uh.abs() @ torch.nan_to_num(ih, posinf=0.0, neginf=0.0).abs().t())
    s[torch.from_numpy(m.toarray() != 0)] = -float('inf')
    order = torch.sort(-s, dim=1, stable=True).indices[:, :k]   # score descending, index ascending within ties
    rs, rt = s.gather(1, order), tol.gather(1, order)
    assert bool((rs > -float('inf')).all())
    val, idx = out[2][0].cpu().double(), out[2][1].cpu().long()
    assert int(idx.min()) >= 0 and int(idx.max()) < I
    inf_pos = rs == float('inf')
    assert int(inf_pos.sum()) > U // 2 and int(inf_pos.sum(1).max()) == 3       # (item 8000's -inf column scores +inf for a negative user entry)
    assert bool((idx[inf_pos] == order[inf_pos]).all()) and bool((val[inf_pos] == float('inf')).all()), 'the +inf items do not lead the lists in index order'
    ps, pt = s.gather(1, idx), tol.gather(1, idx)
    fin = ~inf_pos
    assert bool(((val - ps).abs()[fin] <= pt[fin]).all()), 'a finite score is off by more than the fp32 rounding bound'
    assert bool(((ps - rs).abs()[fin] <= 2 * torch.maximum(pt, rt)[fin]).all()), 'a list differs from the float64 reference beyond near-ties'
    assert bool((ps > -float('inf')).all()), 'an excluded item or an item with score -inf was listed'
    # fp32-class route: finite items (the same values; the cast-overflow item keeps its finite 1e6, the explicit infinities are left out)
    from test_hip_scorer_f32 import _check_against_truth, _truth
    u32_all = u_all_d.float()
    u32 = u32_all[:U]
    i32_d = i32.to(DEV)
    assert ops.split_bf16x3_supported(i32_d)
    got = _fused_guarded('sbr_score_topk_f32s', u32, ops.split_bf16x3(i32_d), I, k, users, ex, G)
    st, tt = _truth(u32, i32_d, users, m)
    _check_against_truth(got, users, st, tt, k, 0, 'fp32-class route, finite items')
    # ... and what it does with a +inf column: unsupported, reported, and memory-safe
    i_inf = i32_d.clone()
    i_inf[5678, 77] = float('inf')
    assert not ops.split_bf16x3_supported(i_inf)
    planes = ops.split_bf16x3(i_inf)
    e = planes[:, 5678, 77].float().cpu()
    assert float(e[0]) == float('inf') and bool(torch.isnan(e[1:]).all()), f'planes of +inf: {e.tolist()}'
    got_inf = _fused_guarded('sbr_score_topk_f32s', u32, planes, I, k, users, ex, G)
    assert int(got_inf[1].min()) >= -1 and int(got_inf[1].max()) < I
    listed = int((got_inf[1] == 5678).any(1).sum())
    others_same = int(((got_inf[1] == got[1]) | (got_inf[1] == 5678)).all(1).sum())
    print(f'fp32-class route with a +inf item column: item listed for {listed} of {U} users, {others_same} lists otherwise unchanged')
