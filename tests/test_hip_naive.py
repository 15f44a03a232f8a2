"""csrc/shared_rank.hip on the GPU: sbr_shared_rank_topk and sbr_uniform_rows_f32 against the numpy restatements of tests/naive_ref.py, bit
for bit (integer and selection work: there is no tolerance), the walk against today's route (expanded rows, mask, radix top-k), and
PopularItems / RandomItems through evaluate_recommender_algorithm and gather_recommender_algorithm_results, also in deterministic mode."""
import functools
import importlib

import numpy as np
import pytest
import torch

import naive_ref as R
from hip_testutil import DEV, S, _Buf, _L, call

pytestmark = pytest.mark.gpu

N_ITEMS = (1, 63, 64, 65, 200)
SCORES = ('all_equal', 'two_levels', 'counts', 'zeros', 'neg_inf')
U_IDX = (4, 0, 2, 1, 3, 0, 4, 2)                 # out of order, users repeated


def ks_of(n):
    return sorted({1, 5, 64, 65, n, n + 3})


@functools.lru_cache(maxsize=None)
def score_vector(kind, n):
    rng = np.random.default_rng(1000 + n)
    if kind == 'all_equal':
        s = np.full(n, 0.25)
    elif kind == 'two_levels':
        s = rng.integers(0, 2, size=n) * 0.5 + 0.125
    elif kind == 'counts':                          # integer counts over their sum: the reference's formula, ties and zeros included
        c = rng.integers(0, 6, size=n).astype(np.float64)
        s = c / max(c.sum(), 1.)
    elif kind == 'zeros':
        s = rng.choice(np.array([-1., -0., 0., 1.]), size=n)
        s[0] = -0.                                  # (n = 1: the one entry is a negative zero)
        if n > 1:
            s[-1] = 0.
    else:
        s = rng.integers(0, 4, size=n).astype(np.float64)
        s[rng.integers(0, n)] = -np.inf             # a real entry: ranks last among the scoreable ones and keeps its index
    return s.astype(np.float32)


def exclusions(order, k, seed):
    """the five users of a batch as a CSR over user ids 0..4 (positions ascending and unique within a row)"""
    n = len(order)
    rng = np.random.default_rng(seed)
    boundary = np.array([r for r in range(n) if r < 63 or 64 <= r < 128], dtype=np.int64)          # keeps ranks 63 and 128 (and what follows)
    rows = [np.arange(0),                                                        # 0: nothing excluded
            np.sort(order[:min(k, n)]),                                          # 1: exactly the ranks 0 .. k-1
            np.arange(n),                                                        # 2: everything
            np.sort(rng.permutation(n)[min(3, n):]),                             # 3: all but 3 items
            np.sort(order[boundary])]                                            # 4: kept items on both sides of a 64-rank step boundary
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32), rows


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


@pytest.mark.parametrize('n', N_ITEMS)
def test_shared_rank_topk_equals_the_restatement(n):
    ops = S().ops
    u_idx = np.array(U_IDX)
    for kind in SCORES:
        score = score_vector(kind, n)
        want_order = R.stable_order(score)
        if kind == 'neg_inf':
            with pytest.raises(ValueError, match='non-finite'):
                ops.shared_ranking(dev(score, torch.float32))
            order = dev(want_order, torch.int32)                                 # -inf goes straight to the kernel
        else:
            order = ops.shared_ranking(dev(score, torch.float32))
            assert order.dtype == torch.int32 and np.array_equal(order.cpu().numpy(), want_order), (kind, n)
        for k in ks_of(n):
            indptr, indices, rows = exclusions(want_order, k, seed=n * 1000 + k)
            val, idx = ops.shared_rank_topk(order, dev(score, torch.float32), dev(u_idx, torch.int64), dev(indptr, torch.int64),
                                            dev(indices, torch.int32), k)
            want_val, want_idx = R.shared_rank_topk_ref(score, u_idx, indptr, indices, k)
            assert val.dtype == torch.float32 and idx.dtype == torch.int32 and tuple(val.shape) == tuple(idx.shape) == (len(u_idx), k)
            got_val, got_idx = val.cpu().numpy(), idx.cpu().numpy()
            assert np.array_equal(got_idx, want_idx), (kind, n, k)
            assert np.array_equal(got_val.view(np.int32), want_val.view(np.int32)), (kind, n, k)
            # what the users were built for
            by_user = {u: b for b, u in enumerate(U_IDX)}
            assert got_idx[by_user[0], :min(k, n)].tolist() == want_order[:min(k, n)].tolist()
            assert got_idx[by_user[1], 0] == (want_order[k] if k < n else -1)
            assert (got_idx[by_user[2]] == -1).all() and np.isneginf(got_val[by_user[2]]).all()
            assert (got_idx[by_user[3]] >= 0).sum() == min(k, 3, n)
            if n == 200:
                assert got_idx[by_user[4], 0] == want_order[63] and (k < 2 or got_idx[by_user[4], 1] == want_order[128])
            if kind == 'neg_inf' and k >= n:
                last = int(np.flatnonzero(np.isneginf(score))[0])
                assert got_idx[by_user[0], n - 1] == last and np.isneginf(got_val[by_user[0], n - 1])      # with its index, not with -1
            for b in (1, 5):                                                     # the repeated users got the same rows
                assert np.array_equal(got_idx[b], got_idx[by_user[U_IDX[b]]])


def test_shared_rank_topk_writes_its_rows_only_and_passes_over_a_bad_entry():
    """raw entry point: identity users (NULL u_idx), outputs inside guarded buffers, an `order` with entries that are no positions"""
    n, k, Bu = 70, 9, 6
    score = score_vector('counts', n)
    order = R.stable_order(score)
    indptr, indices, _ = exclusions(order, k, seed=5)
    indptr = np.concatenate([indptr, [indptr[-1]]])                              # a sixth user without exclusions
    vb, ib = _Buf(Bu, k, off=1), _Buf(Bu, k, off=3, dtype=torch.int32)
    bad = order.copy()
    bad[2], bad[66] = n, -7                                                      # passed over: never read through
    s_dev, ip_dev, ix_dev = dev(score, torch.float32), dev(indptr, torch.int64), dev(indices, torch.int32)      # alive across the raw calls
    for o in (order, bad):
        o_dev = dev(o, torch.int32)
        call('sbr_shared_rank_topk', o_dev.data_ptr(), s_dev.data_ptr(), n, None, ip_dev.data_ptr(), ix_dev.data_ptr(), Bu, k, vb.ptr, ib.ptr,
             _L().stream())
        got_val, got_idx = vb.check_untouched(None, what='out_val').numpy(), ib.check_untouched(None, what='out_idx').numpy()
        keep = (o >= 0) & (o < n)
        want_val, want_idx = R.shared_rank_topk_ref(score, np.arange(Bu), indptr, indices, n)
        for b in range(Bu):
            ranked = [p for p in want_idx[b] if p >= 0 and p in set(o[keep].tolist())][:k]
            assert got_idx[b, :len(ranked)].tolist() == ranked and (got_idx[b, len(ranked):] == -1).all(), b
            assert np.array_equal(got_val[b, :len(ranked)], score[ranked]) and np.isneginf(got_val[b, len(ranked):]).all()
    none = torch.empty(0, dtype=torch.int64, device=DEV)
    val, idx = S().ops.shared_rank_topk(dev(order, torch.int32), dev(score, torch.float32), none, dev(indptr, torch.int64),
                                        dev(indices, torch.int32), 4)
    assert tuple(val.shape) == tuple(idx.shape) == (0, 4)                        # no users: no launch


def test_shared_rank_topk_argument_errors():
    ops = S().ops
    score, order = torch.zeros(5, device=DEV), torch.arange(5, device=DEV, dtype=torch.int32)
    u, indptr, indices = torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV)
    for args, word in (((order.long(), score, u, indptr, indices, 3), 'order'), ((order[:4], score, u, indptr, indices, 3), 'order'),
                       ((order, score.double(), u, indptr, indices, 3), 'score'), ((order, score, u.int(), indptr, indices, 3), 'u_idx'),
                       ((order, score, u, indptr.int(), indices, 3), 'excl_indptr'), ((order, score, u, indptr, indices.long(), 3), 'excl_indices'),
                       ((order, score, u, indptr, indices, 0), 'k='), ((order, score, u, indptr, indices, 2.5), 'k='),
                       ((order[::2], score[::2], u, indptr, indices, 1), 'contiguous')):
        with pytest.raises(ValueError, match=word):
            ops.shared_rank_topk(*args)
    with pytest.raises(ValueError, match='score'):
        ops.shared_ranking(torch.zeros(2, 2, device=DEV))
    with pytest.raises(ValueError, match='non-finite'):
        ops.shared_ranking(torch.tensor([0., float('nan')], device=DEV))
    assert ops.shared_ranking(torch.zeros(0, device=DEV)).shape == (0,)


def test_offsets_past_2_to_31():
    """Bu * k > 2^31 output elements: the rows behind the 2^31st element are the rows in front of it"""
    ops = S().ops
    n, k = 64, 4096
    Bu = (1 << 31) // k + 8
    score = score_vector('counts', n)
    order = R.stable_order(score)
    indptr, indices, _ = exclusions(order, 5, seed=9)
    u = torch.arange(Bu, device=DEV, dtype=torch.int64) % 5
    val, idx = ops.shared_rank_topk(dev(order, torch.int32), dev(score, torch.float32), u, dev(indptr, torch.int64), dev(indices, torch.int32), k)
    assert val.numel() > 1 << 31
    want_val, want_idx = R.shared_rank_topk_ref(score, np.arange(5), indptr, indices, k)
    behind = -(-((1 << 31) // k) // 5) * 5                                       # the first row of user 0 that starts at or past element 2^31
    assert behind * k >= 1 << 31 and behind + 5 <= Bu
    for rows in (slice(0, 5), slice(behind, behind + 5)):                        # users 0..4, in front of and behind 2^31
        assert int(u[rows][0]) == 0 and np.array_equal(idx[rows].cpu().numpy(), want_idx)
        assert np.array_equal(val[rows].cpu().numpy().view(np.int32), want_val.view(np.int32))
    assert bool((idx[-1] == idx[(Bu - 1) % 5]).all()) and bool((idx[:, n:] == -1).all())
    del val, idx
    torch.cuda.empty_cache()


@pytest.mark.parametrize('n', (63, 65, 200))
def test_the_walk_agrees_with_mask_and_topk_rows(n):
    """today's route — the row expanded per user, ops.mask_scores_, ops.topk_rows — gives the same (val, idx) on each user's first
    min(k, scoreable) slots (behind them that route lists masked items, the walk empty slots)"""
    ops = S().ops
    u_idx = np.array(U_IDX)
    for kind in SCORES[:4]:
        score = score_vector(kind, n)
        s_dev = dev(score, torch.float32)
        order = ops.shared_ranking(s_dev)
        for k in sorted({1, 5, 64, min(n, 256)} & set(range(1, n + 1))):
            indptr, indices, rows = exclusions(order.cpu().numpy(), k, seed=n + k)
            u, ip, ix = dev(u_idx, torch.int64), dev(indptr, torch.int64), dev(indices, torch.int32)
            val, idx = ops.shared_rank_topk(order, s_dev, u, ip, ix, k)
            expanded = s_dev.expand(len(u_idx), n).contiguous()
            ops.mask_scores_(expanded, u, ip, ix)
            old_val, old_idx = ops.topk_rows(expanded, k)
            for b, user in enumerate(U_IDX):
                m = min(k, n - len(rows[user]))
                assert torch.equal(idx[b, :m], old_idx[b, :m]), (kind, n, k, b)
                assert bool((val[b, :m] == old_val[b, :m]).all()), (kind, n, k, b)     # (topk_rows returns either zero as +0.0)
                assert bool((idx[b, m:] == -1).all())


# ---- the models ------------------------------------------------------------------------------------------------------------------------
KS = (1, 5, 10, 20)


@functools.lru_cache(maxsize=None)
def world():
    Sm = S()
    ds = Sm.SyntheticDataset(300, 200, 6000, holdout_per_user=2, item_popularity=1.0)
    return ds, ds.eval_view()


def evaluator(view):
    Sm = S()
    return Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=KS), dataset=view)


def loader(view):
    return type('L', (), {'dataset': view, 'batch_size': 64})()


def popular_metrics():
    """-> the metrics of PopularItems by the three scorers, with the hook switched off, and from the restatement's lists"""
    Sm = S()
    ds, view = world()
    out = {}
    for scorer in ('fp32', 'fp16_fused', 'fp32_fused'):
        alg = Sm.PopularItems.build_from_conf({}, ds)
        out[scorer] = Sm.evaluate_recommender_algorithm(alg, loader(view), evaluator(view), DEV, scorer=scorer, user_chunk=77)
    alg = Sm.PopularItems.build_from_conf({}, ds)
    alg.topk_lists = None
    out['hook off'] = Sm.evaluate_recommender_algorithm(alg, loader(view), evaluator(view), DEV, user_chunk=77)
    excl = view.exclude_data.tocsr()
    excl.sort_indices()
    _, idx = R.shared_rank_topk_ref(alg.pop_distribution.cpu().numpy(), view.users_in_split, excl.indptr, excl.indices, max(KS))
    ev = evaluator(view)
    ev.eval_topk(dev(view.users_in_split, torch.int64), dev(idx, torch.int32))
    out['restatement'] = ev.get_results()
    return out


def random_dumps():
    Sm = S()
    _, view = world()

    def dump(seed, **kw):
        d = Sm.gather_recommender_algorithm_results(Sm.RandomItems(seed=seed), loader(view), evaluator(view), device=DEV, **kw)
        return np.asarray(d['topk_item_indices']), np.asarray(d['topk_logits'])
    return dump(3, user_chunk=7), dump(3), dump(3), dump(4)


def test_popular_items_through_the_evaluation():
    got = popular_metrics()
    first = got['fp32']
    assert set(first) >= {f'{m}@{k}' for m in ('ndcg', 'recall', 'precision', 'coverage') for k in KS} and first['ndcg@10'] > 0
    for name, metrics in got.items():
        assert metrics == first, name
    Sm = S()
    ds, view = world()
    alg = Sm.PopularItems.build_from_conf({}, ds)
    d = Sm.gather_recommender_algorithm_results(alg, loader(view), evaluator(view), device=DEV)
    excl = view.exclude_data.tocsr()
    val, idx = R.shared_rank_topk_ref(alg.pop_distribution.cpu().numpy(), view.users_in_split, excl.indptr, excl.indices, max(KS))
    assert np.array_equal(np.asarray(d['topk_item_indices']), idx.astype(np.int64)) and np.array_equal(np.asarray(d['topk_logits']), val)
    assert d['metrics'] == first
    # predict and the hooks: the same fp32 values
    i_idxs = torch.from_numpy(np.random.default_rng(2).integers(0, 200, size=(16, 9)))
    pred = alg.predict(torch.arange(16), i_idxs)
    assert pred.dtype == torch.float32 and torch.equal(pred.cpu(), alg.pop_distribution.cpu()[i_idxs])
    full = alg.combine_user_item_representations(alg.get_user_representations(torch.arange(3)), alg.get_item_representations(torch.arange(200)))
    assert tuple(full.shape) == (3, 200) and full.is_contiguous() and torch.equal(full[2], alg.pop_distribution)


@pytest.mark.parametrize('n', (1, 3, 4, 5, 1000))
def test_uniform_rows_equal_the_restatement(n):
    Sm = S()
    ids = [0, 7, (1 << 31) + 5, 7]
    for seed in (0, 3, (1 << 64) - 1):
        rows = Sm.ops.uniform_rows(seed, dev(np.array(ids), torch.int64), n)
        assert rows.dtype == torch.float32 and tuple(rows.shape) == (4, n)
        want = R.uniform_rows_ref(seed, ids, n)
        assert np.array_equal(rows.cpu().numpy().view(np.int32), want.view(np.int32)), (seed, n)
        for b, u in enumerate(ids):                                              # one user at a time: the same rows
            assert torch.equal(Sm.ops.uniform_rows(seed, dev(np.array([u]), torch.int64), n)[0], rows[b])
        assert torch.equal(rows[1], rows[3])
    # the raw entry point on a row stride that is no multiple of four, off the 16-byte boundary: the element stores, the same bits
    buf = _Buf(4, n, ld=n + 3, off=1)
    ids_dev = dev(np.array(ids), torch.int64)
    call('sbr_uniform_rows_f32', 3, ids_dev.data_ptr(), 4, n, buf.ptr, buf.ld, _L().stream())
    assert np.array_equal(buf.check_untouched(None, what='out').numpy().view(np.int32), R.uniform_rows_ref(3, ids, n).view(np.int32))
    m = Sm.RandomItems(seed=3)
    i_idxs = torch.from_numpy(np.random.default_rng(n).integers(0, n, size=(4, 6)))
    assert torch.equal(m.predict(torch.tensor(ids), i_idxs).cpu(), torch.gather(torch.from_numpy(R.uniform_rows_ref(3, ids, n)), 1, i_idxs))


def test_uniform_rows_range_mean_and_grid_strides():
    ops = S().ops
    rows = ops.uniform_rows(11, torch.arange(1000, device=DEV), 1000)
    assert rows.numel() == 10 ** 6 and bool((rows >= 0).all()) and bool((rows < 1).all())
    mean = float(rows.double().mean())
    print(f'mean of 10^6 values: {mean:.6f}, |mean - 0.5| = {abs(mean - 0.5):.2e}, bound {5 / np.sqrt(12e6):.2e}')
    assert abs(mean - 0.5) < 5 / np.sqrt(12e6)                                  # five standard deviations of the mean
    # more blocks of four than the launch has threads (2^24): the same values as from launches of one row
    Bu, n = 4200, 16001
    assert Bu * ((n + 3) // 4) > 1 << 24
    u = torch.arange(Bu, device=DEV) * 3
    big = ops.uniform_rows(5, u, n)
    for b in (0, 1, 2099, Bu - 1):
        assert torch.equal(big[b], ops.uniform_rows(5, u[b:b + 1], n)[0]), b
    assert np.array_equal(big[Bu - 1].cpu().numpy(), R.uniform_rows_ref(5, [3 * (Bu - 1)], n)[0])
    assert ops.uniform_rows(5, u[:0], n).shape == (0, n) and ops.uniform_rows(5, u[:3], 0).shape == (3, 0)
    for args, word in (((-1, u, 4), 'seed'), ((1 << 64, u, 4), 'seed'), ((0, u.int(), 4), 'u_idx'), ((0, u, -1), 'n_items'), ((0, u[::2], 4), 'contiguous')):
        with pytest.raises(ValueError, match=word):
            ops.uniform_rows(*args)


def test_random_items_lists_do_not_depend_on_the_chunking():
    chunked, whole, again, other = random_dumps()
    assert chunked[0].shape == (300, max(KS)) and (chunked[0] >= 0).all() and (chunked[1] >= 0).all() and (chunked[1] < 1).all()
    for a, b in zip(chunked, whole):
        assert np.array_equal(a, b)
    for a, b in zip(whole, again):
        assert np.array_equal(a, b)
    assert not np.array_equal(whole[0], other[0]) and not np.array_equal(whole[1], other[1])
    _, view = world()
    excl = view.exclude_data.tocsr()
    val, idx = R.shared_rank_topk_ref(R.uniform_rows_ref(3, [17], 200)[0], [0], np.array([0, excl[17].nnz]), excl[17].indices, max(KS))
    assert np.array_equal(whole[0][17], idx[0]) and np.array_equal(whole[1][17], val[0])               # user 17's list, from the restatements


def test_both_models_in_deterministic_mode():
    ops = S().ops
    want_pop, want_rand = popular_metrics(), random_dumps()
    prev = ops.set_deterministic(True)
    try:
        ops.nondeterministic_launches(reset=True)
        got_pop, got_rand = popular_metrics(), random_dumps()
        torch.cuda.synchronize()
        assert ops.nondeterministic_launches(reset=True) == 0
    finally:
        ops.set_deterministic(prev)
    assert got_pop == want_pop
    for a, b in zip(got_rand, want_rand):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
