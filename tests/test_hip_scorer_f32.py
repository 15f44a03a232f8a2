"""GPU: the fused scorer with fp32-class products (csrc/score_topk_f32s.hip: fp32 user rows split in registers, the item matrix split
once into three exact bf16 planes, six bf16-MFMA partial products per score, exclusion mask and running top-k on chip) against a
float64 product of the same fp32 representations (eval/eval.py:216-222 computes in fp32), against the fp32 GEMM -> mask -> exact top-k
route, and through ``evaluate_recommender_algorithm(scorer='fp32_fused')`` / ``Trainer``.

Tolerance of one score: tol = C * 2^-24 * sum_d |u_d i_d| with C = 64. Sources: the three dropped partial products (<= 2^-23 |u_d i_d|
each term) and the fp32 accumulation of the chain (6 D / 16 MFMAs into one accumulator: 48 at D = 128, each rounding once); C bounds
both with room. Two items whose float64 scores lie within 2 tol of each other may trade places in a list (near-ties); nothing else may."""
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from golden_util import MANIFEST, I as G_I, U as G_U, close, load, product_net, world

pytestmark = pytest.mark.gpu
DEV = 'cuda'
C_TOL = 64.0


def S():
    import sibrar_amd
    return sibrar_amd


def _excl(U, I_total, per, seed, heavy=()):
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


def _fused(u32, i32, k, users=None, ex=None, off=0):
    ops = S().ops
    planes = ops.split_bf16x3(i32)
    if ex is None:
        out = ops.score_topk_f32s(u32, planes, k, item_offset=off)
    else:
        out = ops.score_topk_f32s(u32, planes, k, users, ex[0], ex[1], item_offset=off)
    torch.cuda.synchronize()
    return out


def _truth(u32, i32, rows, m=None, off=0):
    """float64 scores of the sampled users (excluded items -inf) and their tolerances"""
    u = u32[rows].double()
    s = u @ i32.double().t()
    tol = C_TOL * 2.0 ** -24 * (u.abs() @ i32.double().abs().t())
    if m is not None:
        dense = torch.from_numpy(m[rows.cpu().numpy()][:, off:off + i32.shape[0]].toarray() != 0).to(DEV)
        s[dense] = -float('inf')
    return s, tol


def _check_against_truth(got, rows, s, tol, k, off=0, what=''):
    """every listed score within tol of its float64 score, no excluded or duplicated item, the float64 top-k up to near-ties, and
    (-inf, -1) behind the scoreable items of a user that has fewer than k"""
    val, idx = got[0][rows].double(), got[1][rows].long()
    n_ok = (s > -float('inf')).sum(1).clamp(max=k)
    valid = torch.arange(k, device=DEV)[None, :] < n_ok[:, None]
    assert bool(((idx >= 0) == valid).all()), f'{what}: list lengths differ from the scoreable item counts'
    assert bool((idx[~valid] == -1).all()) and bool((val[~valid] == -float('inf')).all()), f'{what}: padding is not (-inf, -1)'
    col = (idx - off).clamp(0, s.shape[1] - 1)
    assert bool(((idx - off)[valid] < s.shape[1]).all()), f'{what}: index outside the shard'
    s_pick, t_pick = s.gather(1, col), tol.gather(1, col)
    assert bool((s_pick[valid] > -float('inf')).all()), f'{what}: an excluded item was listed'
    err = (val - s_pick).abs()
    assert bool((err[valid] <= t_pick[valid]).all()), f'{what}: score error {float((err - t_pick)[valid].max())} over tol'
    srt = idx.sort(1).values
    assert not bool(((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)).any()), f'{what}: an item listed twice'
    tv, ti = torch.topk(s, k, dim=1)
    t_truth = tol.gather(1, ti)
    gap = (s_pick - tv).abs()
    ok = gap <= 2 * torch.maximum(t_pick, t_truth)
    assert bool(ok[valid].all()), f'{what}: a list differs from the float64 top-k beyond near-ties (worst {float(gap[valid].max())})'
    # scores descending, ties by item index ascending
    v, i = got[0][rows], got[1][rows]
    assert bool((v[:, :-1] >= v[:, 1:]).all())
    tie = (v[:, :-1] == v[:, 1:]) & (i[:, 1:] >= 0)
    assert bool((i[:, :-1][tie] < i[:, 1:][tie]).all())


def _rows(U):
    return torch.cat([torch.arange(min(U, 512)), torch.tensor([5, U - 1])]).unique().to(DEV)


def _reps(U, I, D, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(U, D, generator=g) / 8).to(DEV), (torch.randn(I, D, generator=g) / 8).to(DEV)


@pytest.mark.parametrize('U,I,D,k,per,off', [(3000, 20000, 128, 20, 30, 0), (2500, 16384, 64, 10, 0, 0), (1100, 9000, 64, 32, 25, 5000),
                                             (40000, 30011, 128, 20, 50, 0), (9000, 12345, 128, 32, 10, 777), (777, 8192, 128, 1, 5, 0),
                                             (33000, 8700, 64, 20, 40, 100)])
def test_f32s_scorer_against_float64_truth(U, I, D, k, per, off):
    """User counts with remainder units and part waves, catalogues that end inside a tile, D = 64 and 128, k = 1 .. 32, a shard that
    starts at item_offset != 0, heavy exclusion rows (users 5 and U - 1)."""
    u32, i32 = _reps(U, I, D, U + I)
    users = torch.arange(U, device=DEV)
    m, ex = _excl(U, off + I + 100, per, U, heavy=((5, 3000), (U - 1, 6000))) if per else (None, None)
    got = _fused(u32, i32, k, users, ex, off)
    rows = _rows(U)
    s, tol = _truth(u32, i32, rows, m, off)
    _check_against_truth(got, rows, s, tol, k, off, f'{U}x{I}x{D} k={k}')
    assert int(got[1].min()) >= -1 and int(got[1].max()) < off + I


def test_f32s_scorer_with_degenerate_users():
    """a user with 5 scoreable items, a user with none, a zero user row (all scores 0: the first k items), exact duplicate items"""
    U, I, D, k = 600, 10000, 128, 20
    u32, i32 = _reps(U, I, D, 3)
    u32[7] = 0
    i32[2000:6000] = i32[0:4000].clone()
    rng = np.random.default_rng(1)
    rows_, cols = [], []
    for u in range(U):
        c = np.setdiff1d(np.arange(I), [3, 4000, 4001, 9998, 9999]) if u == 11 else (np.arange(I) if u == 12 else rng.integers(0, I, size=20))
        rows_.append(np.full(len(c), u)); cols.append(c)
    m = sp.csr_matrix((np.ones(sum(len(r) for r in rows_), dtype=np.int8), (np.concatenate(rows_), np.concatenate(cols))), shape=(U, I))
    m.sum_duplicates(); m.sort_indices()
    ex = S().evaluation._csr_to_device(m, DEV)
    got = _fused(u32, i32, k, torch.arange(U, device=DEV), ex)
    assert got[1][12].tolist() == [-1] * k and got[0][12].tolist() == [-float('inf')] * k
    assert got[1][11, 5:].tolist() == [-1] * (k - 5) and sorted(got[1][11, :5].tolist()) == [3, 4000, 4001, 9998, 9999]
    rows = torch.arange(U, device=DEV)
    s, tol = _truth(u32, i32, rows, m)
    _check_against_truth(got, rows, s, tol, k, 0, 'degenerate users')
    z = got[1][7]
    assert got[0][7].tolist() == [0.0] * k and z.tolist() == sorted(z.tolist())


def test_f32s_scorer_against_the_fp32_route():
    """>= 99.95 % of all list positions identical to the fp32 GEMM -> mask -> exact top-k route (20x tighter than the 1 % the fp16
    route is allowed), and every differing position a near-tie by the float64 rule."""
    U, I, D, k = 20000, 30011, 128, 20
    u32, i32 = _reps(U, I, D, 11)
    users = torch.arange(U, device=DEV)
    m, ex = _excl(U, I, 50, 7)
    got = _fused(u32, i32, k, users, ex)
    ops = S().ops
    same, total = 0, 0
    for lo in range(0, U, 5000):
        r = torch.arange(lo, lo + 5000, device=DEV)
        sc = ops.ScoreAllFn.apply(u32[r], i32)
        ops.mask_scores_(sc, users[r], ex[0], ex[1])
        rv, ri = ops.topk_rows(sc, k)
        gi = got[1][r]
        diff = gi != ri
        same += int((~diff).sum())
        total += diff.numel()
        bad_rows = diff.any(1).nonzero().flatten()
        if bad_rows.numel():
            rows = r[bad_rows]
            s, tol = _truth(u32, i32, rows, m)
            a, b = gi[bad_rows].long(), ri[bad_rows].long()
            sa, sb = s.gather(1, a), s.gather(1, b)
            t = torch.maximum(tol.gather(1, a), tol.gather(1, b))
            d = diff[bad_rows]
            assert bool(((sa - sb).abs() <= 2 * t)[d].all()), 'a position differs from the fp32 route beyond a near-tie'
    assert same / total >= 0.9995, f'{total - same} of {total} positions differ from the fp32 route'


def test_f32s_scorer_on_scores_outside_the_fp16_range():
    """an item whose scores are ~1e6 (no fp16 value; legal in fp32) and Bu % 32 != 0: the lists are the float64 truth's"""
    U, I, D, k = 1013, 5000, 128, 10
    u32, i32 = _reps(U, I, D, 29)
    i32[777] = i32[777] * 4e6
    i32[4999] = -i32[4999] * 2e6
    got = _fused(u32, i32, k)
    rows = torch.arange(U, device=DEV)
    s, tol = _truth(u32, i32, rows)
    _check_against_truth(got, rows, s, tol, k, 0, 'large scores')
    assert float(got[0].max()) > 2e5 and bool((got[1] == 777).any()) and bool((got[1] == 4999).any())


def test_f32s_eight_item_shards_merged_equal_the_unsharded_pass():
    """eight item shards scored at their offsets, stacked as an all-gather leaves them and merged by sbr_merge_topk == one unsharded pass"""
    from importlib import import_module
    _lib = import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')
    U, I, D, k, W = 20_000, 200_000, 128, 20, 8
    u32, i32 = _reps(U, I, D, 5)
    _, ex = _excl(U, I, 50, 5)
    users = torch.arange(U, device=DEV)
    full_v, full_i = _fused(u32, i32, k, users, ex)
    vals = torch.empty(W, U, k, device=DEV, dtype=torch.float32)
    idxs = torch.empty(W, U, k, device=DEV, dtype=torch.int32)
    for r in range(W):
        lo, hi = S().parallel.item_shard(I, r, W)
        vals[r], idxs[r] = _fused(u32, i32[lo:hi].contiguous(), k, users, ex, lo)
    out_v, out_i = torch.empty(U, k, device=DEV), torch.empty(U, k, device=DEV, dtype=torch.int32)
    _lib.call('sbr_merge_topk', vals.data_ptr(), idxs.data_ptr(), W, U, k, out_v.data_ptr(), out_i.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert torch.equal(out_i, full_i) and torch.equal(out_v, full_v), 'sharded + merged differs from the unsharded pass'
    assert int(full_i.min()) >= 0 and int(full_i.max()) < I


# ---- through evaluate_recommender_algorithm / Trainer ----------------------------------------------------------------------------
def _eval(alg, view, scorer, top_k=(1, 10, 20), **kw):
    ev = S().FullEvaluator(config=S().evaluation._Cfg(top_k=top_k, calculate_std=False), dataset=view)
    loader = type('L', (), {'dataset': view, 'batch_size': 64})()
    return S().evaluate_recommender_algorithm(alg, loader, ev, DEV, return_raw=True, scorer=scorer, **kw)


def _assert_same_metrics(a, b, what, tie_users=0):
    (ma, ra), (mb, rb) = a, b
    assert list(ma) == list(mb), what
    for k in ra:
        n_diff = int((ra[k] != rb[k]).sum())
        assert n_diff <= tie_users, f'{what}: per-user {k} differs for {n_diff} users'
    for k in ma:
        if tie_users == 0:
            assert ma[k] == mb[k], f'{what}: {k} {ma[k]} vs {mb[k]}'
        else:
            assert abs(ma[k] - mb[k]) <= 2e-6 * tie_users, f'{what}: {k} {ma[k]} vs {mb[k]}'


def _g9_view(z):
    w = world(z)
    return SimpleNamespace(n_users=G_U, n_items=G_I, items_in_split=np.arange(G_I), users_in_split=np.arange(G_U), n_items_in_split=G_I,
                           n_users_in_split=G_U, user_sampling_matrix=sp.csr_matrix(z['labels']), exclude_data=w['inter'].astype(bool))


def _g9_net(z, D):
    ds = SimpleNamespace(n_users=G_U, n_items=G_I, user_features={}, item_features={
        'text': S().HostFeature('text', 'dense', world(z)['text'])}, user_sampling_matrix_train=world(z)['inter'],
        item_sampling_matrix_train=world(z)['inter_t'], is_cold_start_user=False, is_cold_start_item=False)
    cfg = {'shared_common_dim': D, 'user': {'feature_name': 'user_embedding', 'embedding_dim': -1},
           'item': {'features': [{'feature_name': 'text'}, {'feature_name': 'interactions'}], 'single_branch_hidden_layers': [D],
                    'preference_hidden_layers': [], 'common_modality_dim': D}}
    torch.manual_seed(D)
    return S().SingleBranchNet(S().SingleBranchNetConfig.from_dict(cfg), ds).to(DEV).eval()


@pytest.mark.parametrize('D', [64, 128])
def test_f32s_evaluation_equals_fp32_evaluation_on_the_golden_world(D):
    """The G9 world (50 users x 40 items) with a D-wide model on its own fp32 representations: identical per-user metrics."""
    z = load('g9_eval')
    view = _g9_view(z)
    net = _g9_net(z, D)
    _assert_same_metrics(_eval(net, view, 'fp32'), _eval(net, view, 'fp32_fused'), f'golden world, D = {D}')


def test_f32s_golden_d8_model_falls_back_and_reproduces_the_golden_metrics():
    z = load('g9_eval')
    net = product_net(z, MANIFEST['g9_eval'], 'sd/')
    metrics, raw = _eval(net, _g9_view(z), 'fp32_fused')
    for k in (1, 10, 20):
        for name in ('ndcg', 'recall', 'precision'):
            close(raw[f'{name}@{k}'], z[f'{name}@{k}'], what=f'{name}@{k}', rtol=1e-5, atol=1e-6)
            assert abs(metrics[f'{name}@{k}'] - float(z[f'{name}@{k}'].mean())) < 1e-6


def _world_net(n_users, n_items, nnz, D, seed=5, train_steps=0):
    ds = S().SyntheticDataset(n_users, n_items, nnz, item_dense={'text': 48}, item_tags={'genres': (12, 3)}, seed=seed,
                              n_negative_samples=5, holdout_per_user=2)
    cfg = {'shared_common_dim': D, 'user': {'feature_name': 'user_embedding', 'embedding_dim': -1},
           'item': {'features': [{'feature_name': 'text'}, {'feature_name': 'genres'}, {'feature_name': 'item_embedding'}],
                    'single_branch_hidden_layers': [D], 'preference_hidden_layers': [], 'common_modality_dim': D}}
    torch.manual_seed(seed)
    np.random.seed(seed)
    net = S().SingleBranchNet(S().SingleBranchNetConfig.from_dict(cfg), ds).to(DEV)
    if train_steps:
        net.train()
        loss = S().RecBayesianPersonalizedRankingLoss(n_items=n_items, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=5)
        fused = S().FusedTrainStep(net, loss, S().FusedOptimizer(net, 'adamw', lr=3e-3, weight_decay=1e-6))
        loader = S().NegativeSamplingDataLoader(ds, batch_size=2048, shuffle=True, device=DEV, max_batches=train_steps)
        for b in loader:
            fused.step(*b)
        fused.close()
    net.eval()
    return ds, net


def test_f32s_evaluation_on_a_20k_user_world():
    """20k users x 6k items, D = 128, briefly trained, UNROUNDED representations: the fused fp32-class evaluation matches the fp32
    evaluation user by user except for at most 3 users whose lists hold a near-tie (the two routes sum the same products in another
    order); user_chunk = 7000 (3 launches, the last ragged) equals the single launch; k > 32 falls back to the fp32 route."""
    ds, net = _world_net(20_000, 6_000, 400_000, 128, train_steps=40)
    view = ds.eval_view()
    fp32 = _eval(net, view, 'fp32')
    fused = _eval(net, view, 'fp32_fused')
    assert fp32[0]['ndcg@10'] > 0
    _assert_same_metrics(fp32, fused, 'unrounded representations', tie_users=3)
    _assert_same_metrics(fused, _eval(net, view, 'fp32_fused', user_chunk=7000), 'chunked launches')
    wide = (1, 10, 50)
    _assert_same_metrics(_eval(net, view, 'fp32', top_k=wide), _eval(net, view, 'fp32_fused', top_k=wide), 'k > 32 fall-back')


def test_f32s_through_the_trainer(tmp_path):
    """a Trainer configured with ``scorer: fp32_fused`` runs val() and reports the fp32 scorer's metrics"""
    ds, net = _world_net(900, 700, 20_000, 64, seed=3)
    loss = S().RecBayesianPersonalizedRankingLoss(n_items=ds.n_items, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=5)
    ev = ds.eval_view()
    res = {}
    for scorer in ('fp32', 'fp32_fused'):
        conf = {'learn': {'lr': 5e-3, 'wd': 1e-6, 'optimizer': 'adamw', 'n_epochs': 1, 'optimizing_metric': 'ndcg@10'},
                'run_settings': {'device': DEV, 'batch_verbose': False}, 'results_path': str(tmp_path),
                'eval': S().evaluation._Cfg(top_k=(1, 10, 20)), 'train_eval': None, 'scorer': scorer, 'fused_step': False}
        train_loader = S().NegativeSamplingDataLoader(ds, batch_size=256, shuffle=True, device=DEV)
        val_loader = type('L', (), {'dataset': ev, 'batch_size': 128})()
        tr = S().Trainer(net, train_loader, val_loader, loss, conf)
        assert tr.scorer == scorer
        res[scorer] = tr.val()
        train_loader.close()
    assert res['fp32'] == res['fp32_fused'], (res['fp32'], res['fp32_fused'])
    assert res['fp32']['ndcg@10'] > 0
