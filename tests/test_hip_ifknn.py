"""csrc/dense_knn.hip on the GPU: sbr_dense_knn_topk bit for bit against the numpy float32 restatement on integer features (exact dots),
against the float64 values of tests/ifknn_ref.py under its bound and list rule on float features, by row range, on strided operands
with NaN around them, its argument errors, and ItemFeatureKNN against the g25 fixture recorded from the reference and through
evaluate_recommender_algorithm. The raw runs keep F inside a NaN-filled buffer (leading dimension d + 3, three NaN rows behind row n)
and the outputs in guarded buffers (integer outputs in fp32-typed buffers, read through an int32 view)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import evalk_ref as E
import ifknn_ref as R
from hip_testutil import DEV, S, _Buf, _L, _p, call

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000


def _untouched_bits(buf, written_rows, what):
    bits = buf.flat.cpu().view(torch.int32)
    may = torch.zeros(bits.shape, dtype=torch.bool)
    buf._view(may)[written_rows] = True
    assert bool((bits[~may] == NAN_BITS).all()), f'{what}: elements outside the addressed rows were written'


def run_dense(f, k, shrinkage=0., rows=None, pad=3):
    """raw sbr_row_norms_f32 + sbr_dense_knn_topk on a numpy float32 matrix -> (idx int32 [n, k], val fp32 [n, k], len int32 [n]) as
    numpy, guards checked. F sits in a NaN-filled buffer: ``pad`` NaN columns behind every row and ``pad`` NaN rows behind the last."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    n, d = f.shape
    r0, r1 = (0, n) if rows is None else rows
    fb = _Buf(n + pad, d, ld=d + pad, off=1)
    fb.t[:n].copy_(torch.from_numpy(f).to(DEV))
    norms = _Buf(n, 1)
    call('sbr_row_norms_f32', fb.ptr, n, d, d + pad, norms.ptr, _L().stream())
    norms.check_untouched(what='norms')
    idx, val, length = _Buf(n, k, off=1), _Buf(n, k, off=3), _Buf(n, 1)
    call('sbr_dense_knn_topk', fb.ptr, norms.ptr, n, d, d + pad, r0, r1, float(shrinkage), k, idx.ptr, val.ptr, length.ptr, _L().stream())
    for b, nm in ((idx, 'nbr_idx'), (val, 'nbr_val'), (length, 'nbr_len')):
        _untouched_bits(b, slice(r0, r1), nm)
    return (idx.host().contiguous().view(torch.int32).numpy(), val.host().contiguous().numpy(),
            length.host().contiguous().view(torch.int32).numpy().ravel())


def _same_bits(got, want, what):
    for g, w, nm in zip(got, want, ('idx', 'val', 'len')):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and np.array_equal(g.view(np.int32), w.view(np.int32)), \
            f'{what}: {nm} differs in {int((g.view(np.int32) != w.view(np.int32)).sum())} places'


# ---- bit-exact pin on integer features ---------------------------------------------------------------------------------------------------
def integer_features(n, d, nonneg, seed):
    """integers in [-4, 4] (``nonneg``: [0, 4]) with, as far as n allows, a zero row, a duplicated row, a row that is the negative of
    another (with ``nonneg`` its dots are all <= 0: its list is the self 0, then negative values)"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0 if nonneg else -4, 5, (n, d)).astype(np.float32)
    if n >= 2:
        f[n - 1] = -f[0]
    if n >= 5:
        f[n // 2] = 0
        f[n // 3] = f[1]
    return f


EXACT = [(1, 1, 1, False, 0.), (2, 3, 5, False, 0.), (2, 100, 100, True, 2.5), (63, 32, 5, True, 0.), (63, 1, 256, False, 0.),
         (64, 33, 100, False, 2.5), (65, 100, 1, False, 0.), (130, 3, 256, False, 0.), (130, 33, 5, True, 2.5), (257, 1, 5, False, 0.),
         (257, 32, 100, True, 0.), (257, 100, 256, False, 0.)]


@pytest.mark.parametrize('n,d,k,nonneg,shrinkage', EXACT)
def test_exact_on_integer_features(n, d, k, nonneg, shrinkage):
    """every product and partial sum is exact in fp32, so the dot does not depend on the order: lists, values and lengths equal the numpy
    float32 restatement of the header's operation order bit for bit, ties (d = 1: every value is +-1) included; n < k included"""
    f = integer_features(n, d, nonneg, 100 * n + d)
    got = run_dense(f, k, shrinkage)
    _same_bits(got, R.lists_f32_exact(f, k, shrinkage), f'n={n} d={d} k={k}')
    if n >= 5:
        assert got[2][n // 2] == 0                                                       # the zero row has no candidates
        if nonneg and f[0].any():
            assert got[0][n - 1, 0] == n - 1 and got[1][n - 1, 0] == 0 and not (got[1][n - 1, 1:got[2][n - 1]] > 0).any()


@pytest.mark.parametrize('k', [5, 256])
def test_all_rows_identical(k):
    """every value ties: each list is the lowest indices in order (the row itself with the value 0 comes after the others, which have
    the value 1) — the index passes of the select, over three column tiles"""
    n = 300
    f = np.tile(np.array([[1, -2, 3, 0, 1, 2, -1, 4]], dtype=np.float32), (n, 1))
    idx, val, length = run_dense(f, k)
    _same_bits((idx, val, length), R.lists_f32_exact(f, k), f'identical rows k={k}')
    for i in (0, 3, 299):
        want = [j for j in range(n) if j != i][:k]
        assert idx[i].tolist() == want and (val[i] == 1).all()


# ---- float features -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float_world(n, d):
    for seed in range(n + d, n + d + 20):
        f = np.random.default_rng(seed).normal(size=(n, d)).astype(np.float32)
        f[5] = 0
        f[n - 2] = f[3]                                                                  # identical rows: identical values everywhere
        dot, s_abs, _ = R.dots(f)
        # the first seed at which the fp32 dot of no candidate can round to 0: the candidates are then the same in fp32 and float64
        if not ((dot != 0) & (np.abs(dot) <= R.gamma(d) * s_abs)).any():
            break
    else:
        raise AssertionError('no seed gives candidates that every precision agrees on')
    v, cand = R.values(f)
    return f, v, cand, R.value_bound(f)


@pytest.mark.parametrize('n,d,k', [(400, 24, 100), (400, 100, 100), (3000, 8, 256)])
def test_float_features_meet_the_bound(n, d, k):
    """n = 3000, k = 256: 24 column tiles, so every row carries its list through several reductions of a full buffer"""
    f, v, cand, b = float_world(n, d)
    idx, val, length = run_dense(f, k)
    R.check_kernel_lists(idx, val, length, v, cand, b, k, what=f'n={n} d={d}')
    # value_ij and value_ji carry the same bits where both are listed; identical rows get identical values against every third row
    bits = np.full((n, n), -1, dtype=np.int64)
    r = np.repeat(np.arange(n), k)[(idx >= 0).ravel()]
    bits[r, idx[idx >= 0]] = val.view(np.int32)[idx >= 0]
    both = (bits >= 0) & (bits.T >= 0)
    assert both.sum() > n and np.array_equal(bits[both], bits.T[both])
    third = (bits[3] >= 0) & (bits[n - 2] >= 0)
    third[[3, n - 2]] = False
    assert third.sum() > 0 and np.array_equal(bits[3][third], bits[n - 2][third])


def test_row_range_and_repeat():
    """edges inside a 32-row tile; the range's rows equal the full run bit for bit, the others are untouched (run_dense checks the
    guard pattern); two runs give equal bits"""
    f, _, _, _ = float_world(400, 24)
    f = f[:130]
    full = run_dense(f, 5)
    part = run_dense(f, 5, rows=(30, 101))
    _same_bits([a[30:101] for a in part], [a[30:101] for a in full], 'rows 30..101')
    _same_bits(run_dense(f, 5), full, 'repeat')
    empty = run_dense(f, 5, rows=(40, 40))
    assert (empty[2].view(np.int32) == NAN_BITS).all()


def test_ops_strided_rows_and_deterministic_mode():
    """ops.dense_knn_topk on a strided view inside a NaN buffer equals the run on a contiguous copy, by row range as well, with
    deterministic mode on; the other rows of a ranged result are empty"""
    ops = S().ops
    f, _, _, _ = float_world(400, 24)
    f = torch.from_numpy(f[:130])
    big = torch.full((140, 32), float('nan'), device=DEV)
    big[:130, :24] = f.to(DEV)
    view = big[:130, :24]
    assert view.stride() == (32, 1)
    prev = ops.set_deterministic(True)
    try:
        want = ops.dense_knn_topk(f.to(DEV), 7, 0.)
        got = ops.dense_knn_topk(view, 7, 0.)
        part = ops.dense_knn_topk(view, 7, 0., rows=(33, 97))
    finally:
        ops.set_deterministic(bool(prev))
    _same_bits([t.cpu().numpy() for t in got], [t.cpu().numpy() for t in want], 'strided')
    _same_bits([t[33:97].cpu().numpy() for t in part], [t[33:97].cpu().numpy() for t in want], 'ops rows')
    out = torch.ones(130, dtype=torch.bool)
    out[33:97] = False
    assert (part[0][out] == -1).all() and (part[1][out] == 0).all() and (part[2][out] == 0).all()
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32 and got[0].shape == (130, 7)
    with pytest.raises(ValueError, match='float32'):
        ops.dense_knn_topk(f.double().to(DEV), 7)
    with pytest.raises(ValueError, match='unit column stride'):
        ops.dense_knn_topk(big.t()[:24, :130], 7)
    with pytest.raises(ValueError, match='row range'):
        ops.dense_knn_topk(view, 7, rows=(5, 131))
    bad = f.clone().to(DEV)
    bad[4, 4] = float('inf')
    with pytest.raises(ValueError, match='not finite'):
        ops.dense_knn_topk(bad, 7)
    bad[4, 4] = 3e19                                                                     # the sum of squares overflows
    with pytest.raises(ValueError, match='not finite'):
        ops.dense_knn_topk(bad, 7)
    with pytest.raises(ValueError, match='dense_cosine|unknown similarity'):
        ops.knn_topk(None, 'dense_cosine', 3)


def test_library_errors():
    """argument checks only: every call returns before a launch"""
    Sm = S()
    f = torch.zeros(8, 4, device=DEV)
    nrm = torch.zeros(8, device=DEV)
    idx, val, ln = torch.zeros(8, 256, dtype=torch.int32, device=DEV), torch.zeros(8, 256, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV)
    st = _L().stream()

    def topk(F=f, norms=nrm, n=8, d=4, ld=4, r0=0, r1=8, shrinkage=0., k=3, i=idx, v=val, l=ln):
        call('sbr_dense_knn_topk', _p(F), _p(norms), n, d, ld, r0, r1, shrinkage, k, _p(i), _p(v), _p(l), st)

    for kw, msg in (({'k': 0}, 'k=0'), ({'k': 257}, 'k=257'), ({'d': 0}, 'd=0'), ({'d': 8193, 'ld': 8193}, 'd=8193'), ({'ld': 3}, 'leading dimension'),
                    ({'shrinkage': -1.}, 'negative shrinkage'), ({'r0': 5, 'r1': 4}, 'row range'), ({'r1': 9}, 'row range'), ({'r0': -1}, 'row range'),
                    ({'F': None}, 'null'), ({'norms': None}, 'null'), ({'i': None}, 'null'), ({'v': None}, 'null'), ({'l': None}, 'null'),
                    ({'n': 1 << 24, 'k': 128, 'r1': 8}, '2\\^31')):
        with pytest.raises(Sm.SibrarHipError, match='sbr_dense_knn_topk.*' + msg):
            topk(**kw)
    topk(r0=3, r1=3, F=None)                                                             # an empty range returns before the operands are looked at
    for args, msg in (((_p(f), 8, 0, 4, _p(nrm)), 'bad shape'), ((_p(f), 8, 4, 3, _p(nrm)), 'bad shape'), ((None, 8, 4, 4, _p(nrm)), 'null'),
                      ((_p(f), 8, 4, 4, None), 'null')):
        with pytest.raises(Sm.SibrarHipError, match='sbr_row_norms_f32.*' + msg):
            call('sbr_row_norms_f32', *args, st)
    assert (idx == 0).all() and (ln == 0).all()


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
ARRAYS, CASES = R.load_g25()


def _model(case):
    return S().KNNAlgorithm.build_from_conf({'alg': 'ifknn', 'k': case['k'], 'shrinkage': case['shrinkage'],
                                             'sim_func_params': {'sim_func_name': 'dense_cosine'}}, None)


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_model_meets_the_reference(case):
    inter = sp.csr_matrix(ARRAYS['inter'])
    f = R.case_features(case, ARRAYS)
    m = _model(case).fit(inter, f if case['k'] == 5 else torch.from_numpy(f))
    n_users, n_items = inter.shape
    pred = m.combine_user_item_representations(m.get_user_representations(torch.arange(n_users)), m.get_item_representations(torch.arange(n_items)))
    assert pred.shape == (n_users, n_items)
    R.check_case_against_fixture(case, ARRAYS, m.nbr_idx.cpu().numpy(), m.nbr_val.cpu().numpy(), m.nbr_len.cpu().numpy(), pred.cpu().numpy(),
                                 fp32=True)
    if case['features'] == 'signed' and case['k'] == 60:
        val, ln = m.nbr_val.cpu().numpy(), m.nbr_len.cpu().numpy()
        assert ln[7] == 0 and (ln[np.arange(40) != 7] == 39).all() and val.min() < -0.5  # the self 0 and the negative values are kept


def test_predict_round_trip_and_foreign_file(tmp_path):
    Sm = S()
    case = next(c for c in CASES if c['name'] == 'ifknn_signed_s0_k5')
    inter = sp.csr_matrix(ARRAYS['inter'])
    m = _model(case).fit(inter, sp.csr_matrix(ARRAYS['features']))
    rng = np.random.default_rng(3)
    u = torch.from_numpy(rng.integers(0, 50, size=16))
    i = torch.from_numpy(rng.integers(0, 40, size=(16, 9)))
    full = m.combine_user_item_representations(m.get_user_representations(u), m.get_item_representations(torch.arange(40)))
    got = m.predict(u, i)
    assert got.shape == (16, 9) and torch.equal(got, torch.gather(full, 1, i.to(DEV)))
    indptr, indices, data, shape = m.similarity_csr()
    s = sp.csr_matrix((data.cpu().numpy(), indices.cpu().numpy(), indptr.cpu().numpy()), shape=shape).toarray()
    assert np.array_equal(s, R.lists_to_dense(m.nbr_idx.cpu().numpy(), m.nbr_val.cpu().numpy(), m.nbr_len.cpu().numpy()).astype(np.float32))
    m.save_model_to_path(str(tmp_path))
    back = _model(case)
    back.load_model_from_path(str(tmp_path))
    with pytest.raises(RuntimeError, match='attach'):
        back.predict(u, i)
    back.attach(inter)
    assert torch.equal(back.predict(u, i), got)
    other = tmp_path / 'iknn'
    other.mkdir()
    Sm.ItemKNN(Sm.SimilarityFunctionEnum.cosine, k=5).fit(inter).save_model_to_path(str(other))
    with pytest.raises(ValueError, match='ItemKNN'):
        _model(case).load_model_from_path(str(other))
    with pytest.raises(ValueError, match='ItemFeatureKNN'):
        Sm.ItemKNN(Sm.SimilarityFunctionEnum.cosine, k=5).load_model_from_path(str(tmp_path))


@functools.lru_cache(maxsize=None)
def eval_world():
    """dataset, fitted model and, from the float64 restatement, the top-10 of every evaluated user with the users whose first eleven
    masked float64 scores lie further apart than the fp32 score error could bridge"""
    Sm = S()
    ds = Sm.SyntheticDataset(300, 200, 4000, seed=6, n_negative_samples=3, holdout_per_user=1)
    f = np.random.default_rng(9).normal(size=(200, 16)).astype(np.float32)
    k = 20
    m = Sm.ItemFeatureKNN(k=k).fit(ds.user_sampling_matrix_train, f)
    v64, cand = R.values(f)
    assert not R.boundary_tied(v64, cand, k).any()
    idx, val, ln = R.lists(v64, cand, k)
    assert np.array_equal(np.sort(m.nbr_idx.cpu().numpy(), 1), np.sort(idx, 1))          # no row tied at the k-th place: the same sets
    x = np.asarray(sp.csr_matrix(ds.user_sampling_matrix_train).todense())
    pred = R.predict(R.lists_to_dense(idx, val, ln), x)
    tol = R.predict(np.abs(R.lists_to_dense(idx, R.value_bound(f)[np.arange(200)[:, None], np.maximum(idx, 0)], ln)), x)
    tol = tol + R.gamma(k * x.sum(axis=1, keepdims=True)) * R.predict(np.abs(R.lists_to_dense(idx, val, ln)), x)
    return ds, m, pred, tol


@pytest.mark.parametrize('scorer', ['fp32', 'fp16_fused'])
def test_evaluate_recommender_algorithm(scorer):
    """both scorers take the fp32 route for this model; the metrics equal those of the float64 restatement's top-k on the untied users"""
    Sm = S()
    ds, m, pred, tol = eval_world()
    view = ds.eval_view()
    ks = (1, 5, 10)
    ev = Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=ks, metrics=('ndcg', 'recall', 'precision')), dataset=view)
    loader = type('L', (), {'dataset': view, 'batch_size': 64})()
    kw = {} if scorer == 'fp32' else {'scorer': scorer}
    metrics, raw = Sm.evaluate_recommender_algorithm(m, loader, ev, DEV, return_raw=True, user_chunk=128, **kw)
    users = np.asarray(view.users_in_split)
    items = np.asarray(view.items_in_split)
    excl = sp.csr_matrix(view.exclude_data)
    excl.sort_indices()
    masked = pred[users][:, items].copy()
    for b, u in enumerate(users):
        masked[b, excl.indices[excl.indptr[u]:excl.indptr[u + 1]]] = -np.inf
    order = np.argsort(-masked, axis=1, kind='stable')[:, :max(ks) + 1]
    top_v = np.take_along_axis(masked, order, 1)
    gap = 2 * np.take_along_axis(tol[users][:, items], order, 1).max(axis=1)
    untied = np.isfinite(top_v).all(axis=1) & ((top_v[:, :-1] - top_v[:, 1:]).min(axis=1) > gap)
    assert untied.sum() >= 0.5 * len(users)
    lab = sp.csr_matrix(view.user_sampling_matrix)[:, items]
    lab.sort_indices()
    got = np.stack([np.stack([raw[f'{name}@{k}'] for k in ks]) for name in ('ndcg', 'recall', 'precision')])
    E.check_metrics(got[:, :, untied], order[untied, :max(ks)].astype(np.int32), users[untied], (lab.indptr, lab.indices), ks, what=f'ifknn {scorer}')
    assert metrics['ndcg@10'] == pytest.approx(float(got[0, 2].mean()), rel=1e-6)
