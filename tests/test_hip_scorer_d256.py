"""GPU: the fp32-class fused scorer for 256-wide representations (``ops.score_topk_f32s_d256``, ``fused_max_d=256``)
against float64, item-sharded, and through ``evaluate_recommender_algorithm`` / ``gather_recommender_algorithm_results``.

Rules: tests/scorer_truth_util.py (every listed score within tol = C * 2^-24 * sum_d |u_d i_d| of float64; a list is the float64 top-k
except where two float64 scores lie within 2 tol; no excluded or duplicated item; (-inf, -1) padding).

The constant at D = 256 is C = 128. The module's C = 64 for D <= 128 covers (a) the three partial products the six-term sum drops, each
at most 2^-23 |u_d i_d| = 2 * 2^-24 |u_d i_d|: 6 units of 2^-24 sum |u_d i_d|, whatever D is, and (b) the fp32 accumulation of the chain:
6 D / 16 MFMAs into one accumulator, each adding at most one rounding of a partial sum that is itself bounded by sum |u_d i_d|: 48 units
at D = 128, 54 in all, bounded with room by 64. At D = 256 the chain is 6 * 256 / 16 = 96 MFMAs: (a) stays 6, (b) doubles to 96, 102 in
all, bounded the same way by 128. Nothing here is taken from what the kernel returns."""
import numpy as np
import pytest
import torch

from scorer_truth_util import DEV, S, check_against_truth, csr_of, excl, reps, sample_rows, truth
from test_hip_scorer_wide import _eval, _fused_calls, _gather, _lib, _logged, _near_tie_users, _world_net

pytestmark = pytest.mark.gpu
C256 = 128.0
D = 256


def fused256(u32, i32, k, users=None, ex=None, off=0):
    ops = S().ops
    planes = ops.split_bf16x3(i32)
    out = ops.score_topk_f32s_d256(u32, planes, k, item_offset=off) if ex is None else \
        ops.score_topk_f32s_d256(u32, planes, k, users, ex[0], ex[1], item_offset=off)
    torch.cuda.synchronize()
    return out


HEAVY = 'heavy'
CASES = [  # U, I, k, exclusions per user, item_offset, heavy rows (users 5 and U - 1: 3,000 and 6,000 entries)
    (3001, 20000, 20, 30, 0, HEAVY),                    # Bu % 32 != 0
    (3001, 20000, 100, 30, 0, HEAVY),
    (2500, 16384, 32, 0, 0, None),                      # no exclusions, catalogue = whole tiles
    (2500, 16384, 33, 0, 0, None),
    (1100, 9000, 33, 25, 5000, HEAVY),                  # shard at item_offset != 0
    (1100, 9000, 1, 25, 5000, HEAVY),
    (40000, 30011, 100, 50, 0, HEAVY),                  # several workgroups per CU; catalogue ends inside a tile
    (40000, 30011, 32, 50, 0, HEAVY),
    (9000, 12345, 128, 10, 777, HEAVY),                 # remainder units in parts (one full wave + a part wave per workgroup)
    (9000, 12345, 20, 10, 777, HEAVY),
    (20000, 8700, 20, 40, 100, HEAVY),                  # remainder units in parts (two full waves + a part wave), prefix pass
    (20000, 8700, 128, 40, 100, HEAVY),
    (777, 1500, 1, 5, 0, None),                         # Bu % 32 != 0; catalogue below the prefix-pass size
    (777, 1500, 20, 5, 0, None),
    (777, 1500, 100, 5, 0, None),
    (1013, 150, 100, 150, 0, None),                     # catalogue shorter than k + exclusions: padded lists
    (1013, 150, 128, 150, 0, None),
    (1013, 40, 32, 30, 0, None),
    (37, 8192, 20, 5, 0, None),                         # fewer users than one workgroup's
]


@pytest.mark.parametrize('U,I,k,per,off,heavy', CASES)
def test_d256_scorer_against_float64_truth(U, I, k, per, off, heavy):
    u32, i32 = reps(U, I, D, U + I + k)
    users = torch.arange(U, device=DEV)
    m, ex = excl(U, off + I + 100, per, U, heavy=((5, 3000), (U - 1, 6000)) if heavy else ()) if per else (None, None)
    got = fused256(u32, i32, k, users, ex, off)
    rows = sample_rows(U)
    s, tol = truth(u32, i32, rows, m, off, C256)
    check_against_truth(got, rows, s, tol, k, off, f'd256 {U}x{I} k={k}')
    assert int(got[1].min()) >= -1 and int(got[1].max()) < off + I


def test_d256_scorer_with_degenerate_users():
    """k = 100: a user with 5 scoreable items, one with none, one with exactly k, a zero user row (all scores 0: the first k scoreable
    item positions in order), 4,000 exact duplicate item rows (ties at the threshold: the smallest indices stay)"""
    U, I, k = 600, 10000, 100
    u32, i32 = reps(U, I, D, 3)
    u32[7] = 0
    i32[2000:6000] = i32[0:4000].clone()
    rng = np.random.default_rng(1)
    keep13 = np.sort(rng.choice(I, size=k, replace=False))
    rows_, cols = [], []
    for u in range(U):
        if u == 11:
            c_ = np.setdiff1d(np.arange(I), [3, 4000, 4001, 9998, 9999])
        elif u == 12:
            c_ = np.arange(I)
        elif u == 13:
            c_ = np.setdiff1d(np.arange(I), keep13)
        else:
            c_ = rng.integers(0, I, size=20)
        rows_.append(np.full(len(c_), u)); cols.append(c_)
    m, ex = csr_of(rows_, cols, (U, I))
    got = fused256(u32, i32, k, torch.arange(U, device=DEV), ex)
    assert got[1][12].tolist() == [-1] * k and got[0][12].tolist() == [-float('inf')] * k
    assert got[1][11, 5:].tolist() == [-1] * (k - 5) and sorted(got[1][11, :5].tolist()) == [3, 4000, 4001, 9998, 9999]
    assert sorted(got[1][13].tolist()) == keep13.tolist()
    rows = torch.arange(U, device=DEV)
    s, tol = truth(u32, i32, rows, m, 0, C256)
    check_against_truth(got, rows, s, tol, k, 0, 'd256 degenerate users')
    first = np.setdiff1d(np.arange(I), m[7].indices)[:k]
    assert got[0][7].tolist() == [0.0] * k and got[1][7].tolist() == first.tolist()
    # exact duplicates: items j and j + 2000 (j < 2000) have the same bits; wherever the copy is listed, the original is listed before it
    idx = got[1].long()
    for u in (0, 1, 100, 599):
        lst = idx[u].tolist()
        for p_, it in enumerate(lst):
            if 2000 <= it < 4000 and not m[u, it - 2000]:
                assert it - 2000 in lst[:p_], f'user {u}: item {it} listed without its smaller-index duplicate'


def test_d256_wide_lists_extend_the_narrow_lists_bit_for_bit():
    """a score's bits do not depend on k: the k = 100 list starts with the k = 32 list, the k = 128 list with the k = 100 list"""
    U, I = 3000, 20000
    u32, i32 = reps(U, I, D, 1)
    users = torch.arange(U, device=DEV)
    _, ex = excl(U, I, 30, 1, heavy=((5, 3000),))
    l32, l100, l128 = (fused256(u32, i32, k, users, ex) for k in (32, 100, 128))
    assert torch.equal(l100[0][:, :32], l32[0]) and torch.equal(l100[1][:, :32], l32[1])
    assert torch.equal(l128[0][:, :100], l100[0]) and torch.equal(l128[1][:, :100], l100[1])


def test_d256_c5_shard_shape_against_float64_truth():
    """the item shard of BASELINE configs[4] as one rank sees it: 100k users x 25k items x 256 at item_offset 75,000, k = 20, 50
    exclusions per user over the whole 200k catalogue; sampled rows against float64"""
    U, I, k, off = 100_000, 25_000, 20, 75_000
    u32, i32 = reps(U, I, D, 9)
    users = torch.arange(U, device=DEV)
    m, ex = excl(U, 200_000, 50, 9, heavy=((5, 3000), (U - 1, 6000)))
    got = fused256(u32, i32, k, users, ex, off)
    rows = torch.cat([sample_rows(U), torch.arange(50_000, 50_256, device=DEV), torch.arange(U - 300, U, device=DEV)]).unique()
    s, tol = truth(u32, i32, rows, m, off, C256)
    check_against_truth(got, rows, s, tol, k, off, 'd256 c5 shard')
    assert int(got[1].min()) >= off and int(got[1].max()) < off + I


def test_d256_eight_item_shards_merged_equal_the_unsharded_pass():
    """eight item shards of a 200k x 256 catalogue scored at their offsets, stacked as an all-gather leaves them and merged by
    sbr_merge_topk == one unsharded pass of the same route, bit for bit"""
    lib = _lib()
    U, I, k, W = 20_000, 200_000, 20, 8
    u32, i32 = reps(U, I, D, 5)
    _, ex = excl(U, I, 50, 5)
    users = torch.arange(U, device=DEV)
    full_v, full_i = fused256(u32, i32, k, users, ex)
    vals = torch.empty(W, U, k, device=DEV, dtype=torch.float32)
    idxs = torch.empty(W, U, k, device=DEV, dtype=torch.int32)
    for r in range(W):
        lo, hi = S().parallel.item_shard(I, r, W)
        assert hi - lo == 25_000
        vals[r], idxs[r] = fused256(u32, i32[lo:hi].contiguous(), k, users, ex, lo)
    out_v, out_i = torch.empty(U, k, device=DEV), torch.empty(U, k, device=DEV, dtype=torch.int32)
    lib.call('sbr_merge_topk', vals.data_ptr(), idxs.data_ptr(), W, U, k, out_v.data_ptr(), out_i.data_ptr(), lib.stream())
    torch.cuda.synchronize()
    assert torch.equal(out_i, full_i) and torch.equal(out_v, full_v), 'sharded + merged differs from the unsharded pass'
    assert int(full_i.min()) >= 0 and int(full_i.max()) < I


def test_d256_launches_are_deterministic_and_the_old_entry_still_refuses():
    U, I, k = 5000, 30000, 100
    u32, i32 = reps(U, I, D, 17)
    users = torch.arange(U, device=DEV)
    _, ex = excl(U, I, 50, 3)
    before = S().ops.nondeterministic_launches()
    a, b = fused256(u32, i32, k, users, ex), fused256(u32, i32, k, users, ex)
    assert S().ops.nondeterministic_launches() == before
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    planes = S().ops.split_bf16x3(i32)
    with pytest.raises(Exception, match='D=256 not supported'):
        S().ops.score_topk_f32s(u32, planes, 20)
    with pytest.raises(Exception, match=r'outside \[1, 128\]'):
        S().ops.score_topk_f32s_d256(u32, planes, 129)
    u128, i128 = reps(64, 500, 128, 1)
    with pytest.raises(ValueError, match='D=128 not supported'):
        S().ops.score_topk_f32s_d256(u128, S().ops.split_bf16x3(i128), 20)


# ---- through evaluate_recommender_algorithm / gather_recommender_algorithm_results -------------------------------------------------
ENTRY = 'sbr_score_topk_f32s_d256'


def test_d256_evaluation_on_a_synthetic_world():
    """8k users x 4k items, a 256-wide model, briefly trained, unrounded representations.
      * scorer='fp32_fused', fused_max_d=256 runs sbr_score_topk_f32s_d256 and no sbr_topk_rows: top-20 lists with the default
        fused_max_k, top-100 lists with fused_max_k=128;
      * per-user metrics equal the fp32 route's except for users whose two dumped lists differ, and those differ at near-tie positions
        only (float64 rule, C = 128);
      * the evaluation returns the dump's metrics, chunked or not, and the dump's lists do not depend on the chunking;
      * with the default fused_max_d the route falls back to the fp32 path as before (sbr_topk_rows, no fused call);
      * non-finite item values fall back as before."""
    ds, net = _world_net(8_000, 4_000, 160_000, D, train_steps=20)
    view = ds.eval_view()
    n_users = len(view.users_in_split)
    for top_k, kw in (((1, 10, 20), dict(fused_max_d=256)), ((1, 10, 50, 100), dict(fused_max_d=256, fused_max_k=128))):
        kmax = max(top_k)
        ref = _gather(net, view, 'fp32', top_k)
        new, log = _logged(lambda: _gather(net, view, 'fp32_fused', top_k, **kw))
        calls = _fused_calls(log, ENTRY)
        assert calls and all(a[10] == kmax and a[2] == D for a in calls), [n for n, _ in log]
        assert not _fused_calls(log, 'sbr_topk_rows') and not _fused_calls(log, 'sbr_score_topk_f32s')
        assert ref['metrics'][f'ndcg@{kmax}'] > 0 and list(ref['metrics']) == list(new['metrics'])
        n_tie = _near_tie_users(net, view, ref, new, C256)
        print(f'\n[d256] fp32_fused vs fp32 through the evaluator, top-{kmax} lists: {n_tie} of {n_users} users differ (near-ties only)')
        ev1 = _eval(net, view, 'fp32_fused', top_k, **kw)
        ev2 = _eval(net, view, 'fp32_fused', top_k, user_chunk=3000, **kw)
        assert ev1[0] == new['metrics'] and ev2[0] == ev1[0]
        for name in ev1[1]:
            assert np.array_equal(ev1[1][name], new['raw_metrics'][name]) and np.array_equal(ev1[1][name], ev2[1][name])
        chunked = _gather(net, view, 'fp32_fused', top_k, user_chunk=3000, **kw)
        assert np.array_equal(chunked['topk_item_indices'], new['topk_item_indices']) and np.array_equal(chunked['topk_logits'], new['topk_logits'])
        # default fused_max_d: today's fall-back
        dkw = {k_: v for k_, v in kw.items() if k_ != 'fused_max_d'}
        dflt, log = _logged(lambda: _eval(net, view, 'fp32_fused', top_k, **dkw))
        assert not _fused_calls(log, ENTRY) and not _fused_calls(log, 'sbr_score_topk_f32s') and _fused_calls(log, 'sbr_topk_rows')
        assert dflt[0] == ref['metrics']
    # a largest cut-off beyond fused_max_k falls back with fused_max_d=256 too
    far, log = _logged(lambda: _eval(net, view, 'fp32_fused', (1, 50), fused_max_d=256))
    assert not _fused_calls(log, ENTRY) and _fused_calls(log, 'sbr_topk_rows') and 'ndcg@50' in far[0]

    class _InfItem(torch.nn.Module):
        def __init__(self, net):
            super().__init__()
            self.net = net

        def get_item_representations(self, i):
            r = self.net.get_item_representations(i).clone()
            r[3, 5] = float('inf')
            return r

        def get_user_representations(self, u):
            return self.net.get_user_representations(u)

        def combine_user_item_representations(self, u, i):
            return self.net.combine_user_item_representations(u, i)

    _, log = _logged(lambda: _eval(_InfItem(net), view, 'fp32_fused', (1, 10, 20), fused_max_d=256))
    assert not _fused_calls(log, ENTRY) and _fused_calls(log, 'sbr_topk_rows')
