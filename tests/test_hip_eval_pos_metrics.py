"""GPU: FullEvaluator with the rank-position metrics (dcg, ap, rr: sbr_rank_metrics_pos) on the split of rankpos_ref.evaluator_world.
The per-user arrays must equal the fp32 restatement (ap and rr bit for bit, dcg inside rankpos_ref.dcg_bound of float64), a default
evaluator must return what it returned before these metrics existed and must not launch the new entry, and the keys must reach every
consumer that needs no new code: _std, groups, raw results, the natural order, eval_batch, evaluate_recommender_algorithm and
gather_recommender_algorithm_results."""
import functools
import types

import numpy as np
import pytest
import torch

import rankpos_ref as R
from hip_testutil import DEV, S, U32, _L, _i64

pytestmark = pytest.mark.gpu

DEFAULT = ('ndcg', 'precision', 'recall', 'f_score', 'hitrate', 'coverage')
POS = ('dcg', 'ap', 'rr')


@functools.lru_cache(maxsize=None)
def world():
    full, items, calls, csr, cat = R.evaluator_world()
    feats = {'gender': S().HostFeature('gender', 'categorical', cat, n_categories=2, unique_values=['F', 'M'])}
    ds = types.SimpleNamespace(user_sampling_matrix=full, items_in_split=items, n_items_in_split=len(items), n_users=full.shape[0],
                               user_features=feats)
    return ds, calls, csr


def _evaluate(metrics=None, name=None, groups=False):
    """both eval_topk calls, then get_results -> (metrics, raw, cut-offs per launch of each metric entry)"""
    ds, calls, _ = world()
    kw = {} if metrics is None else {'metrics': list(metrics)}
    cfg = S().evaluation._Cfg(top_k=list(R.EVAL_KS), calculate_group_metrics=groups, **kw)
    ev = S().FullEvaluator(config=cfg, evaluator_name=name, dataset=ds)
    lib = _L()
    lib.CALL_LOG = []
    try:
        for ids, top in calls:
            ev.eval_topk(_i64(ids), torch.as_tensor(top).to(DEV))
        launches = {entry: [args[7] for nm, args in lib.CALL_LOG if nm == entry] for entry in ('sbr_rank_metrics', 'sbr_rank_metrics_pos')}
    finally:
        lib.CALL_LOG = None
    return ev.get_results(return_raw_results=True) + (launches,)


def _oracle():
    """{key: (float32 per-user restatement, float64 per-user definition, bound)} over the users of both calls in call order"""
    _, calls, csr = world()
    f32 = np.concatenate([R.pos_metrics_f32(top, ids, csr, R.EVAL_KS) for ids, top in calls], axis=2)
    f64 = np.concatenate([R.pos_metrics_ref64(top, ids, csr, R.EVAL_KS) for ids, top in calls], axis=2)
    db = np.concatenate([R.dcg_bound(top, ids, csr, R.EVAL_KS) for ids, top in calls], axis=1)
    return {f'{m}@{k}': (f32[j, q], f64[j, q], db[q] if m == 'dcg' else None) for j, m in enumerate(POS) for q, k in enumerate(R.EVAL_KS)}


def test_new_metrics_equal_the_oracle_in_natural_order():
    from oracle import eval_ref
    metrics, raw, launches = _evaluate(['ndcg', 'dcg', 'ap', 'rr'])
    want = _oracle()
    assert set(raw) == set(want) | {f'ndcg@{k}' for k in R.EVAL_KS}
    assert set(metrics) == set(raw) | {f'{k}_std' for k in raw}
    assert list(metrics) == eval_ref.natural_sorted(list(metrics)), 'the keys are not in natural order'
    assert launches == {'sbr_rank_metrics': [8, 3, 8, 3], 'sbr_rank_metrics_pos': [8, 3, 8, 3]}, launches
    for key, (f32, f64, bound) in want.items():
        got = raw[key]
        assert got.dtype == np.float32 and got.shape == f32.shape, key
        if bound is None:
            assert np.array_equal(got.view(np.int32), f32.view(np.int32)), f'{key}: differs in bits from the fp32 restatement'
            assert metrics[key] == float(f32.mean()) and metrics[f'{key}_std'] == float(f32.std()), f'{key}: mean / _std of the oracle'
        else:
            err = np.abs(got - f64)
            assert (err <= bound).all(), f'{key}: off by up to {err.max():.3e}'
        # the reported mean and _std are those of the returned array (get_results: float(v.mean()), float(v.std()))
        assert metrics[key] == float(got.mean()) and metrics[f'{key}_std'] == float(got.std()), key
        # and lie where the float64 figures put them: an fp32 pairwise mean of 280 values errs by less than 16 u of it; the standard
        # deviation moves by at most the largest per-user error and its fp32 evaluation by less than 16 u (1 + std)
        per_user = np.abs(got - f64).max()
        assert abs(metrics[key] - f64.mean()) <= per_user + 16 * U32 * abs(f64.mean()) + 2.0 ** -149, key
        assert abs(metrics[f'{key}_std'] - f64.std()) <= per_user + 16 * U32 * (1 + f64.std()), key
    assert metrics['ap@10'] > 0 and metrics['rr@70'] >= metrics['rr@1'] and metrics['dcg@70'] >= metrics['dcg@1']


def test_default_config_is_untouched_and_does_not_launch_the_new_entry():
    metrics, raw, launches = _evaluate()
    assert launches == {'sbr_rank_metrics': [8, 3, 8, 3], 'sbr_rank_metrics_pos': []}, launches
    per_user = {f'{m}@{k}' for m in DEFAULT if m != 'coverage' for k in R.EVAL_KS}
    assert set(raw) == per_user
    assert set(metrics) == per_user | {f'{k}_std' for k in per_user} | {f'coverage@{k}' for k in R.EVAL_KS}      # the parent's keys
    assert tuple(S().evaluation._Cfg().metrics) == DEFAULT
    # an evaluator that also computes the new metrics returns the same bits under every one of those keys
    more, more_raw, _ = _evaluate(DEFAULT + POS)
    assert set(more) == set(metrics) | {f'{m}@{k}{s}' for m in POS for k in R.EVAL_KS for s in ('', '_std')}
    for key, value in metrics.items():
        assert more[key] == value, key
    for key, value in raw.items():
        assert np.array_equal(more_raw[key].view(np.int32), value.view(np.int32)), key


def test_group_keys_and_the_evaluator_name_prefix():
    metrics, raw, _ = _evaluate(['ap', 'rr', 'dcg'], name='val', groups=True)
    ds, calls, _ = world()
    cats = np.concatenate([np.asarray(ds.user_features['gender'].values)[ids] for ids, _ in calls])
    for m in POS:
        for k in R.EVAL_KS:
            whole = raw[f'val/{m}@{k}']
            for c, label in enumerate(('f', 'm')):
                key = f'val/gender_{label}/{m}@{k}'
                assert np.array_equal(raw[key], whole[cats == c]), key
                assert metrics[key] == float(whole[cats == c].mean()) and f'{key}_std' in metrics
    assert not any(k.split('/')[-1].startswith(('ndcg', 'recall', 'coverage')) for k in metrics)


def test_eval_batch_reports_the_new_metrics():
    """the dense entry point: scores that rank a user's list first give that list, hence the oracle's figures"""
    ds, calls, csr = world()
    ids, top = calls[0][0][:50], calls[0][1][:50]
    top = top[:, :20]
    keep = (top >= 0).all(axis=1)                                 # dense scores cannot express an empty slot
    ids, top = ids[keep], top[keep]
    scores = np.zeros((len(ids), 400), dtype=np.float32)
    scores[np.arange(len(ids))[:, None], top] = np.arange(20, 0, -1, dtype=np.float32)[None, :]
    ev = S().FullEvaluator(config=S().evaluation._Cfg(top_k=[1, 5, 20], metrics=['ap', 'rr', 'dcg']), dataset=ds)
    ev.eval_batch(_i64(ids), torch.from_numpy(scores).to(DEV))
    _, raw = ev.get_results(return_raw_results=True)
    want = R.pos_metrics_f32(top, ids, csr, [1, 5, 20])
    for j, m in enumerate(POS):
        for q, k in enumerate([1, 5, 20]):
            if m == 'dcg':
                assert (np.abs(raw[f'dcg@{k}'] - R.pos_metrics_ref64(top, ids, csr, [1, 5, 20])[0, q]) <= R.dcg_bound(top, ids, csr, [1, 5, 20])[q]).all()
            else:
                assert np.array_equal(raw[f'{m}@{k}'].view(np.int32), want[j, q].view(np.int32)), f'{m}@{k}'


def test_models_through_the_evaluation_and_the_dump():
    Sm = S()
    ds = Sm.SyntheticDataset(300, 400, 9000, holdout_per_user=2, item_popularity=1.0)
    view = ds.eval_view()
    loader = type('L', (), {'dataset': view, 'batch_size': 64})()
    ks = (1, 10, 300)                                             # a list longer than the 256 entries sbr_topk_rows serves
    keys = {f'{m}@{k}' for m in POS for k in ks}

    def evaluator(top_k):
        return Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=top_k, metrics=['ndcg', 'ap', 'rr', 'dcg']), dataset=view)

    pop = Sm.PopularItems.build_from_conf({}, ds)
    metrics, raw = Sm.evaluate_recommender_algorithm(pop, loader, evaluator(ks), DEV, return_raw=True, user_chunk=77)
    assert keys <= set(raw) and keys | {f'{k}_std' for k in keys} <= set(metrics)
    assert all(raw[k].shape == (len(view.users_in_split),) for k in keys)
    assert 0 < metrics['ap@10'] <= 1 and 0 < metrics['rr@300'] <= 1 and metrics['dcg@300'] >= metrics['dcg@10'] > 0
    # the same figures from the model's own lists through the oracle
    excl = Sm.evaluation._csr_to_device(view.exclude_data, DEV)
    users = np.asarray(view.users_in_split).astype(np.int64)
    _, idx = pop.topk_lists(_i64(users), _i64(np.asarray(view.items_in_split)), excl[0], excl[1], 300)
    import scipy.sparse as sp
    lab = sp.csr_matrix(view.user_sampling_matrix)[:, np.asarray(view.items_in_split)]
    lab.sort_indices()
    csr = (lab.indptr.astype(np.int64), lab.indices.astype(np.int32))
    want = R.pos_metrics_f32(idx.cpu().numpy(), users, csr, list(ks))
    for j, m in enumerate(('ap', 'rr')):
        for q, k in enumerate(ks):
            assert np.array_equal(raw[f'{m}@{k}'].view(np.int32), want[1 + j, q].view(np.int32)), f'PopularItems {m}@{k}'
    torch.manual_seed(5)
    mf = Sm.SGDMatrixFactorization(ds.n_users, ds.n_items, 16).to(DEV)
    small = (1, 10, 50)
    metrics, raw = Sm.evaluate_recommender_algorithm(mf, loader, evaluator(small), DEV, return_raw=True)
    assert {f'{m}@{k}' for m in POS for k in small} <= set(raw)
    assert all(0 <= metrics[f'{m}@{k}'] <= 1 for m in ('ap', 'rr') for k in small)
    dump = Sm.gather_recommender_algorithm_results(mf, loader, evaluator(small), device=DEV)
    assert {f'{m}@{k}' for m in POS for k in small} <= set(dump['raw_metrics']) and dump['metrics'] == metrics
    for k in raw:
        assert np.array_equal(dump['raw_metrics'][k], raw[k]), k


def test_unknown_metrics_still_raise_and_name_the_nine():
    with pytest.raises(ValueError, match='not supported') as info:
        S().FullEvaluator(config=S().evaluation._Cfg(metrics=['map']))
    for name in DEFAULT + POS:
        assert f"'{name}'" in str(info.value), name
    assert len(S().evaluation.SUPPORTED_METRICS) == 9
