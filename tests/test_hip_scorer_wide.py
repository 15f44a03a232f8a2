"""GPU: the wide instantiations of the one-pass fused scorers (lists of 33 .. 128 entries) against float64, against
the k <= 32 kernels, against the fp32 route, item-sharded, through ``evaluate_recommender_algorithm(fused_max_k=128)`` / ``Trainer``,
and the top-k dump ``gather_recommender_algorithm_results``. Tolerances and the near-tie rule: tests/scorer_truth_util.py (the rules of
the k <= 32 tests, unchanged)."""
import importlib
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from golden_util import MANIFEST, I as G_I, U as G_U, load, product_net, world
from scorer_truth_util import DEV, S, check_against_truth, csr_of, excl, fused, operands, reps, sample_rows, truth

pytestmark = pytest.mark.gpu
ROUTES = ('f16', 'f32s')

# share of list positions that differ from the fp32 GEMM -> mask -> radix top-k route at k = 100 (20,000 x 30,011 x 128, 50 exclusions
# per user), measured on one MI355X: 230 of 2,000,000 positions (all of them near-ties by the float64 rule); see
# test_wide_f32s_against_the_fp32_route
D_SHARE_K100 = 230 / 2_000_000


def _lib():
    return importlib.import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')


HEAVY = 'heavy'
CASES = [  # U, I, D, k, exclusions per user, item_offset, heavy rows (users 5 and U - 1: 3,000 and 6,000 entries)
    (3000, 20000, 128, 100, 30, 0, HEAVY),
    (2500, 16384, 64, 50, 0, 0, None),                  # no exclusions, catalogue = whole tiles
    (1100, 9000, 64, 33, 25, 5000, HEAVY),              # shard at item_offset != 0
    (40000, 30011, 128, 64, 50, 0, HEAVY),              # remainder units in parts; catalogue ends inside a tile
    (33000, 8700, 64, 128, 40, 100, HEAVY),             # remainder units in parts
    (9000, 12345, 128, 128, 10, 777, HEAVY),
    (777, 1500, 128, 100, 5, 0, None),                  # Bu % 32 != 0; catalogue below the k <= 32 kernels' prefix-pass size
    (1013, 150, 64, 100, 150, 0, None),                 # catalogue shorter than k + exclusions: padded lists
    (3001, 20000, 256, 100, 30, 0, HEAVY),              # D = 256: fp16 route only
    (40000, 9000, 256, 50, 20, 0, HEAVY),
]


@pytest.mark.parametrize('route', ROUTES)
@pytest.mark.parametrize('U,I,D,k,per,off,heavy', CASES)
def test_wide_scorer_against_float64_truth(route, U, I, D, k, per, off, heavy):
    if route == 'f32s' and D == 256:
        with pytest.raises(Exception, match='D=256 not supported'):
            fused(route, *reps(64, 500, D, 1), k)
        return
    u32, i32 = reps(U, I, D, U + I + k)
    users = torch.arange(U, device=DEV)
    m, ex = excl(U, off + I + 100, per, U, heavy=((5, 3000), (U - 1, 6000)) if heavy else ()) if per else (None, None)
    got = fused(route, u32, i32, k, users, ex, off)
    rows = sample_rows(U)
    ur, ir, c = operands(route, u32, i32)
    s, tol = truth(ur, ir, rows, m, off, c)
    check_against_truth(got, rows, s, tol, k, off, f'{route} {U}x{I}x{D} k={k}')
    assert int(got[1].min()) >= -1 and int(got[1].max()) < off + I


@pytest.mark.parametrize('route', ROUTES)
def test_wide_scorer_with_degenerate_users(route):
    """k = 100: a user with 5 scoreable items, one with none, one with exactly k, a zero user row (all scores 0: the first k scoreable
    item positions in order), 4,000 exact duplicate item rows (ties at the threshold: the smallest indices stay)"""
    U, I, D, k = 600, 10000, 128, 100
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
    got = fused(route, u32, i32, k, torch.arange(U, device=DEV), ex)
    assert got[1][12].tolist() == [-1] * k and got[0][12].tolist() == [-float('inf')] * k
    assert got[1][11, 5:].tolist() == [-1] * (k - 5) and sorted(got[1][11, :5].tolist()) == [3, 4000, 4001, 9998, 9999]
    assert sorted(got[1][13].tolist()) == keep13.tolist()
    rows = torch.arange(U, device=DEV)
    ur, ir, c = operands(route, u32, i32)
    s, tol = truth(ur, ir, rows, m, 0, c)
    check_against_truth(got, rows, s, tol, k, 0, f'{route} degenerate users')
    first = np.setdiff1d(np.arange(I), m[7].indices)[:k]
    assert got[0][7].tolist() == [0.0] * k and got[1][7].tolist() == first.tolist()
    # exact duplicates: items j and j + 2000 (j < 2000) have the same bits; wherever the copy is listed, the original is listed before it
    idx = got[1].long()
    for u in (0, 1, 100, 599):
        lst = idx[u].tolist()
        for p_, it in enumerate(lst):
            if 2000 <= it < 4000 and not m[u, it - 2000]:
                assert it - 2000 in lst[:p_], f'user {u}: item {it} listed without its smaller-index duplicate'


def test_wide_f32s_scorer_on_scores_outside_the_fp16_range():
    """scores of ~1e6 (no fp16 value; legal in fp32) at k = 100 and Bu % 32 != 0: the lists are the float64 truth's"""
    U, I, D, k = 1013, 5000, 128, 100
    u32, i32 = reps(U, I, D, 29)
    i32[777] = i32[777] * 4e6
    i32[4999] = -i32[4999] * 2e6
    got = fused('f32s', u32, i32, k)
    rows = torch.arange(U, device=DEV)
    s, tol = truth(u32, i32, rows)
    check_against_truth(got, rows, s, tol, k, 0, 'large scores')
    assert float(got[0].max()) > 2e5 and bool((got[1] == 777).any()) and bool((got[1] == 4999).any())


@pytest.mark.parametrize('route', ROUTES)
def test_wide_lists_extend_the_narrow_lists_bit_for_bit(route):
    """The first 32 entries of the k = 100 list ARE the k = 32 list (values and indices, torch.equal) and the first 100 of k = 128 are
    the k = 100 list: a score's bits do not depend on k (same MFMA chain in every instantiation) and every list is the exact top-k of
    those scores under one tie rule. Ties the wide kernels to the k <= 32 kernels, which the older tests pin."""
    for (U, I, D, per, seed) in ((3000, 20000, 128, 30, 1), (33000, 8700, 64, 40, 2)):
        u32, i32 = reps(U, I, D, seed)
        users = torch.arange(U, device=DEV)
        _, ex = excl(U, I, per, seed, heavy=((5, 3000),))
        l32, l100, l128 = (fused(route, u32, i32, k, users, ex) for k in (32, 100, 128))
        assert torch.equal(l100[0][:, :32], l32[0]) and torch.equal(l100[1][:, :32], l32[1]), f'{route}: k = 100 does not extend k = 32'
        assert torch.equal(l128[0][:, :100], l100[0]) and torch.equal(l128[1][:, :100], l100[1]), f'{route}: k = 128 does not extend k = 100'


def test_wide_f32s_against_the_fp32_route():
    """k = 100, 20,000 x 30,011 x 128, 50 exclusions per user (the construction of test_f32s_scorer_against_the_fp32_route): every
    position that differs from the fp32 GEMM -> mask -> exact top-k route is a near-tie by the float64 rule. That assertion carries the
    weight. The SHARE of differing positions is not fixed in advance (near-ties get denser deeper in a list); it is measured — see
    D_SHARE_K100 and DESIGN.md 4.6 — and asserted to stay within twice the measurement (inputs are seeded and neither route has float
    atomics: the factor two only absorbs another summation order of the fp32 GEMM on another machine or library version).
    Measured on one MI355X: 230 of 2,000,000 positions differ, d = 0.000115 (k = 20 on the same inputs: at most 0.0005 allowed)."""
    U, I, D, k = 20000, 30011, 128, 100
    u32, i32 = reps(U, I, D, 11)
    users = torch.arange(U, device=DEV)
    m, ex = excl(U, I, 50, 7)
    got = fused('f32s', u32, i32, k, users, ex)
    ops = S().ops
    same, total = 0, 0
    for lo in range(0, U, 5000):
        r = torch.arange(lo, lo + 5000, device=DEV)
        sc = ops.ScoreAllFn.apply(u32[r], i32)
        ops.mask_scores_(sc, users[r], ex[0], ex[1])
        rv, ri = ops.topk_rows(sc, k)
        del sc
        gi = got[1][r]
        diff = gi != ri
        same += int((~diff).sum())
        total += diff.numel()
        bad_rows = diff.any(1).nonzero().flatten()
        for c0 in range(0, bad_rows.numel(), 512):
            br = bad_rows[c0:c0 + 512]
            s, tol = truth(u32, i32, r[br], m)
            a, b = gi[br].long(), ri[br].long()
            sa, sb = s.gather(1, a), s.gather(1, b)
            t = torch.maximum(tol.gather(1, a), tol.gather(1, b))
            d = diff[br]
            assert bool(((sa - sb).abs() <= 2 * t)[d].all()), 'a position differs from the fp32 route beyond a near-tie'
    share = (total - same) / total
    print(f'\n[wide] fp32_fused vs fp32 route at k = 100: {total - same} of {total} positions differ (share {share:.6f})')
    assert share <= 2 * D_SHARE_K100, f'{total - same} of {total} positions differ from the fp32 route (measured share {D_SHARE_K100})'


@pytest.mark.parametrize('route', ROUTES)
def test_wide_eight_item_shards_merged_equal_the_unsharded_pass(route):
    """eight item shards at k = 100, scored at their offsets and merged (parallel.merge_topk: 8 x 100 entries are beyond
    sbr_merge_topk) == one unsharded pass, exactly"""
    U, I, D, k, W = 20_000, 200_000, 128, 100, 8
    u32, i32 = reps(U, I, D, 5)
    _, ex = excl(U, I, 50, 5)
    users = torch.arange(U, device=DEV)
    full_v, full_i = fused(route, u32, i32, k, users, ex)
    vals, idxs = [], []
    for r in range(W):
        lo, hi = S().parallel.item_shard(I, r, W)
        v, i = fused(route, u32, i32[lo:hi].contiguous(), k, users, ex, lo)
        vals.append(v); idxs.append(i)
    out_v, out_i = S().parallel.merge_topk(torch.cat(vals, 1), torch.cat(idxs, 1), k)
    assert torch.equal(out_i.to(full_i.dtype), full_i) and torch.equal(out_v, full_v), 'sharded + merged differs from the unsharded pass'
    assert int(full_i.min()) >= 0 and int(full_i.max()) < I


@pytest.mark.parametrize('route', ROUTES)
def test_wide_launches_are_deterministic(route):
    """two calls on the same inputs at k = 100 return identical bits, and neither is an arrival-order launch"""
    U, I, D, k = 5000, 30000, 128, 100
    u32, i32 = reps(U, I, D, 17)
    users = torch.arange(U, device=DEV)
    _, ex = excl(U, I, 50, 3)
    before = S().ops.nondeterministic_launches()
    a = fused(route, u32, i32, k, users, ex)
    b = fused(route, u32, i32, k, users, ex)
    assert S().ops.nondeterministic_launches() == before
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_two_pass_route_refuses_wide_lists():
    """the opt-in two-pass route stays at k <= 32 and says so instead of running another kernel"""
    u32, i32 = reps(400, 8200, 64, 1)
    prev = S().ops.score_topk_route(2)
    try:
        with pytest.raises(Exception, match='two-pass route takes k <= 32'):
            fused('f16', u32, i32, 33)
    finally:
        S().ops.score_topk_route(prev)
    with pytest.raises(Exception, match=r'outside \[1, 128\]'):
        fused('f16', u32, i32, 129)
    with pytest.raises(Exception, match=r'outside \[1, 128\]'):
        fused('f32s', u32, i32, 129)


# ---- through evaluate_recommender_algorithm / gather_recommender_algorithm_results / Trainer --------------------------------------
class _Fp16Rounded(torch.nn.Module):
    """A model whose representations are already fp16 values (held in fp32): both scorers then see identical inputs."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def get_item_representations(self, i):
        return self.net.get_item_representations(i).half().float()

    def get_user_representations(self, u):
        return self.net.get_user_representations(u).half().float()

    def combine_user_item_representations(self, u, i):
        return self.net.combine_user_item_representations(u, i)

    def check_index_errors(self):
        self.net.check_index_errors()


def _loader(view, bs=64):
    return type('L', (), {'dataset': view, 'batch_size': bs})()


def _eval(alg, view, scorer, top_k, **kw):
    ev = S().FullEvaluator(config=S().evaluation._Cfg(top_k=top_k, calculate_std=False), dataset=view)
    return S().evaluate_recommender_algorithm(alg, _loader(view), ev, DEV, return_raw=True, scorer=scorer, **kw)


def _gather(alg, view, scorer, top_k, bs=64, path=None, **kw):
    ev = S().FullEvaluator(config=S().evaluation._Cfg(top_k=top_k, calculate_std=False), dataset=view)
    return S().gather_recommender_algorithm_results(alg, _loader(view, bs), ev, path, DEV, scorer=scorer, **kw)


def _logged(fn):
    lib = _lib()
    lib.CALL_LOG = []
    try:
        out = fn()
    finally:
        log, lib.CALL_LOG = lib.CALL_LOG, None
    return out, log


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
        step = S().FusedTrainStep(net, loss, S().FusedOptimizer(net, 'adamw', lr=3e-3, weight_decay=1e-6))
        loader = S().NegativeSamplingDataLoader(ds, batch_size=2048, shuffle=True, device=DEV, max_batches=train_steps)
        for b in loader:
            step.step(*b)
        step.close()
    net.eval()
    return ds, net


def _near_tie_users(alg, view, a, b, c):
    """Users whose dumped lists differ -> their number, after checking that EVERY differing position is a near-tie by the float64 rule
    (tolerance constant c on the representations the model hands out); users whose lists are equal have equal metrics."""
    ia, ib = torch.from_numpy(a['topk_item_indices']).to(DEV), torch.from_numpy(b['topk_item_indices']).to(DEV)
    assert np.array_equal(a['user_indices'], b['user_indices'])
    differ = (ia != ib).any(1)
    for name in a['raw_metrics']:
        moved = torch.from_numpy(a['raw_metrics'][name] != b['raw_metrics'][name]).to(DEV)
        assert not bool((moved & ~differ).any()), f'{name}: a user with identical lists has different metrics'
    rows = differ.nonzero().flatten()
    if rows.numel():
        with torch.no_grad():
            items = torch.as_tensor(np.asarray(view.items_in_split)).to(DEV)
            u_ids = torch.from_numpy(a['user_indices']).to(DEV)[rows]
            u = alg.get_user_representations(u_ids).double()
            it = alg.get_item_representations(items).double()
        s = u @ it.t()
        tol = c * 2.0 ** -24 * (u.abs() @ it.abs().t())
        pa, pb = ia[rows], ib[rows]
        sa, sb = s.gather(1, pa), s.gather(1, pb)
        t = torch.maximum(tol.gather(1, pa), tol.gather(1, pb))
        d = pa != pb
        assert bool(((sa - sb).abs() <= 2 * t)[d].all()), 'two lists differ beyond near-ties'
    return int(rows.numel())


def _fused_calls(log, entry):
    return [args for name, args in log if name == entry]


def test_wide_evaluation_on_a_20k_user_world():
    """20k users x 6k items, D = 128, briefly trained, top_k = (1, 10, 50, 100).
      * fused_max_k = 128 keeps 'fp32_fused' (unrounded representations) and 'fp16_fused' (fp16-rounded representations) on their
        kernels with k = 100 and no sbr_topk_rows launch; with the default fused_max_k both fall back to the fp32 route as before;
      * per-user metrics equal the fp32 route's except for users whose two dumped lists differ, and those differ at near-tie positions
        only (checked for every such user). Measured on one MI355X (recorded, not asserted): 101 of 20,000 users for 'fp32_fused',
        74 for 'fp16_fused' on fp16-rounded representations;
      * user_chunk = 7000 equals the single launch exactly; a largest cut-off of 129 falls back."""
    ds, net = _world_net(20_000, 6_000, 400_000, 128, train_steps=40)
    view = ds.eval_view()
    top_k = (1, 10, 50, 100)
    for scorer, alg, entry, c in (('fp32_fused', net, 'sbr_score_topk_f32s', 64.0), ('fp16_fused', _Fp16Rounded(net), 'sbr_score_topk_f16', 128.0)):
        ref = _gather(alg, view, 'fp32', top_k)
        wide, log = _logged(lambda: _gather(alg, view, scorer, top_k, fused_max_k=128))
        calls = _fused_calls(log, entry)
        assert calls and all(a[10] == 100 for a in calls) and not _fused_calls(log, 'sbr_topk_rows'), [n for n, _ in log]
        assert ref['metrics']['ndcg@100'] > 0 and list(ref['metrics']) == list(wide['metrics'])
        n_tie = _near_tie_users(alg, view, ref, wide, c)
        print(f'\n[wide] {scorer} vs fp32 through the evaluator, top-100 lists: {n_tie} of 20000 users differ (near-ties only)')
        # the evaluation proper returns the dump's metrics, chunked or not
        ev1 = _eval(alg, view, scorer, top_k, fused_max_k=128)
        ev2 = _eval(alg, view, scorer, top_k, fused_max_k=128, user_chunk=7000)
        assert ev1[0] == wide['metrics'] and ev2[0] == ev1[0]
        for name in ev1[1]:
            assert np.array_equal(ev1[1][name], wide['raw_metrics'][name]) and np.array_equal(ev1[1][name], ev2[1][name])
        chunked = _gather(alg, view, scorer, top_k, fused_max_k=128, user_chunk=7000)
        assert np.array_equal(chunked['topk_item_indices'], wide['topk_item_indices']) and np.array_equal(chunked['topk_logits'], wide['topk_logits'])
        assert np.array_equal(chunked['targets'], wide['targets'])
        # defaults: the fall-back of today
        dflt, log = _logged(lambda: _eval(alg, view, scorer, top_k))
        assert not _fused_calls(log, entry) and _fused_calls(log, 'sbr_topk_rows')
        assert dflt[0] == ref['metrics']
        # a largest cut-off of 129 is beyond the wide kernels
        far, log = _logged(lambda: _eval(alg, view, scorer, (1, 129), fused_max_k=128))
        assert not _fused_calls(log, entry) and _fused_calls(log, 'sbr_topk_rows') and 'ndcg@129' in far[0]


def test_wide_through_the_trainer(tmp_path):
    """a Trainer with ``scorer: fp32_fused``, ``fused_max_k: 128`` and the reference's default cut-offs (up to 100) runs val() on the
    fused kernel and reports ndcg@100"""
    ds, net = _world_net(900, 700, 20_000, 64, seed=3)
    loss = S().RecBayesianPersonalizedRankingLoss(n_items=ds.n_items, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=5)
    conf = {'learn': {'lr': 5e-3, 'wd': 1e-6, 'optimizer': 'adamw', 'n_epochs': 1, 'optimizing_metric': 'ndcg@10'},
            'run_settings': {'device': DEV, 'batch_verbose': False}, 'results_path': str(tmp_path),
            'eval': S().evaluation._Cfg(), 'train_eval': None, 'scorer': 'fp32_fused', 'fused_max_k': 128, 'fused_step': False}
    train_loader = S().NegativeSamplingDataLoader(ds, batch_size=256, shuffle=True, device=DEV)
    tr = S().Trainer(net, train_loader, _loader(ds.eval_view(), 128), loss, conf)
    assert tr.scorer == 'fp32_fused' and tr.fused_max_k == 128
    res, log = _logged(tr.val)
    train_loader.close()
    calls = _fused_calls(log, 'sbr_score_topk_f32s')
    assert calls and calls[0][10] == 100 and not _fused_calls(log, 'sbr_topk_rows')
    assert 0 < res['ndcg@100'] <= 1 and 'ndcg@50' in res


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


@pytest.mark.parametrize('model', ['golden D=8 (fall-back)', 'D=64 (fused)'])
def test_gather_results_on_the_golden_world(model, tmp_path):
    """The G9 world (50 users x 40 items), reference-default cut-offs (largest 100 -> k = 40 = items of the split): keys, shapes,
    dtypes; lists = torch.topk of the masked float64 scores up to the route's tolerance; metrics = the evaluation's, exactly; targets
    per loader batch of 16 users; the pickle round-trips."""
    z = load('g9_eval')
    view = _g9_view(z)
    fusedp = model.startswith('D=64')
    net = _g9_net(z, 64) if fusedp else product_net(z, MANIFEST['g9_eval'], 'sd/')
    top_k = tuple(S().evaluation._Cfg().top_k)
    path = str(tmp_path / 'dump.pkl')
    kw = dict(scorer='fp32_fused', fused_max_k=128)
    out, log = _logged(lambda: _gather(net, view, top_k=top_k, bs=16, path=path, **kw))
    assert bool(_fused_calls(log, 'sbr_score_topk_f32s')) == fusedp
    assert set(out) == {'n_users', 'n_items', 'k', 'topk_item_indices', 'topk_logits', 'user_indices', 'targets', 'metrics', 'raw_metrics'}
    assert (out['n_users'], out['n_items'], out['k']) == (G_U, G_I, 40)
    assert out['topk_item_indices'].shape == (G_U, 40) and out['topk_item_indices'].dtype == np.int64
    assert out['topk_logits'].shape == (G_U, 40) and out['topk_logits'].dtype == np.float32
    assert out['user_indices'].dtype == np.int64 and out['user_indices'].tolist() == list(range(G_U))
    labels = np.asarray(z['labels']) != 0
    want = np.concatenate([np.argwhere(labels[b:b + 16]) for b in range(0, G_U, 16)])
    assert out['targets'].dtype == np.int64 and np.array_equal(out['targets'], want)
    # lists against float64
    with torch.no_grad():
        rows = torch.arange(G_U, device=DEV)
        u = net.get_user_representations(rows)
        it = net.get_item_representations(torch.arange(G_I, device=DEV))
    m = sp.csr_matrix(view.exclude_data)
    s, tol = truth(u, it, rows, m)
    val, idx = torch.from_numpy(out['topk_logits']).to(DEV), torch.from_numpy(out['topk_item_indices']).to(DEV)
    if fusedp:
        check_against_truth((val, idx), rows, s, tol, 40, 0, 'gathered lists')
    else:
        # the fp32 route lists excluded items (score -inf) behind the scoreable ones instead of empty slots
        s_pick, t_pick = s.gather(1, idx), tol.gather(1, idx)
        fin = s_pick > -float('inf')
        assert bool((fin.sum(1) == (s > -float('inf')).sum(1)).all()) and bool((val[~fin] == -float('inf')).all())
        assert bool(((val.double() - s_pick).abs()[fin] <= t_pick[fin]).all())
        tv, ti = torch.topk(s, 40, dim=1)
        assert bool((((s_pick - tv).abs() <= 2 * torch.maximum(t_pick, tol.gather(1, ti))) | ~fin).all())
        assert bool((val[:, :-1] >= val[:, 1:]).all())
    # metrics: the evaluation's on the same inputs
    metrics, raw = _eval(net, view, top_k=top_k, **kw)
    assert out['metrics'] == metrics and set(out['raw_metrics']) == set(raw)
    for name in raw:
        assert np.array_equal(out['raw_metrics'][name], raw[name])
    back = pickle.load(open(path, 'rb'))
    assert set(back) == set(out) and back['metrics'] == out['metrics'] and back['k'] == 40
    for name in ('topk_item_indices', 'topk_logits', 'user_indices', 'targets'):
        assert np.array_equal(back[name], out[name])
