"""csrc/knn.hip on the GPU: sbr_knn_topk against the float64 values of tests/knn_ref.py under a rule that is tolerant of near-ties,
sbr_csr_rows_times_csr against float64 sums with the bound of an fp32 sum in a fixed order, and UserKNN / ItemKNN against the g22 fixture
recorded from the reference and through evaluate_recommender_algorithm. Operands and outputs sit in the guarded buffers of hip_testutil.py
(integer outputs in fp32-typed buffers, read through an int32 view)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import evalk_ref as E
import knn_ref as R
from hip_testutil import DEV, S, U32, _Buf, _assert_bits, _i32, _i64, _L, _p, call

pytestmark = pytest.mark.gpu

SIM_CODE = {'cosine': 0, 'jaccard': 1, 'asymmetric_cosine': 2, 'sorensen_dice': 3, 'tversky': 4}
PARAMS = {'cosine': {}, 'jaccard': {}, 'asymmetric_cosine': {'alpha': 0.3}, 'tversky': {'alpha': 0.7, 'beta': 0.2}, 'sorensen_dice': {}}
NAN_BITS = 0x7FC00000


def _csr_dev(m):
    m = sp.csr_matrix(m)
    m.sort_indices()
    return _i64(m.indptr), _i32(m.indices)


def _untouched_bits(buf, written_rows, what):
    """every element outside the written rows still holds the fill pattern, bit for bit (-1 is a NaN pattern too: isnan would not do)"""
    bits = buf.flat.cpu().view(torch.int32)
    may = torch.zeros(bits.shape, dtype=torch.bool)
    buf._view(may)[written_rows] = True
    assert bool((bits[~may] == NAN_BITS).all()), f'{what}: elements outside the addressed rows were written'


def run_knn(x, sim, k, shrinkage=0., alpha=0., beta=0., tile_cols=0, rows=None, check=True):
    """raw sbr_knn_topk on a scipy 0/1 matrix -> (idx int32 [n, k], val fp32 [n, k], len int32 [n]) as numpy, guards checked"""
    x = sp.csr_matrix(x)
    n, m = x.shape
    r0, r1 = (0, n) if rows is None else rows
    indptr, indices = _csr_dev(x)
    t_indptr, t_indices = _csr_dev(x.T)
    kb = max(k, 1)                                                    # (k = 0 is an argument error: the buffers still have to exist)
    idx, val, length = _Buf(n, kb, off=1), _Buf(n, kb, off=3), _Buf(n, 1)
    call('sbr_knn_topk', _p(indptr), _p(indices), _p(t_indptr), _p(t_indices), n, m, r0, r1, SIM_CODE[sim], float(alpha or 0.), float(beta or 0.),
         float(shrinkage), k, tile_cols, idx.ptr, val.ptr, length.ptr, _L().stream())
    if check:
        for b, nm in ((idx, 'nbr_idx'), (val, 'nbr_val'), (length, 'nbr_len')):
            _untouched_bits(b, slice(r0, r1), nm)
    return (idx.host().contiguous().view(torch.int32).numpy(), val.host().contiguous().numpy(),
            length.host().contiguous().view(torch.int32).numpy().ravel())


# ---- the 150 x 90 matrix: 8 % density, an empty row, two identical rows ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_matrix():
    rng = np.random.default_rng(22)
    d = rng.random((150, 90)) < 0.08
    d[17] = False                       # an empty row
    d[101] = d[40]                      # two identical rows
    assert d[40].sum() >= 3
    return sp.csr_matrix(d.astype(np.float32))


@functools.lru_cache(maxsize=None)
def small_truth(sim, shrinkage):
    x = small_matrix()
    c = R.counts(x)
    v = R.values(x, sim, shrinkage, PARAMS[sim].get('alpha'), PARAMS[sim].get('beta'), c)
    b = R.value_bound(x, sim, shrinkage, PARAMS[sim].get('alpha'), PARAMS[sim].get('beta'), c, v)
    return sp.csr_matrix(v), sp.csr_matrix(b), v


@pytest.mark.parametrize('tile_cols', [64, 0])
@pytest.mark.parametrize('k', [1, 5, 100, 256])
@pytest.mark.parametrize('shrinkage', [0., 5.])
@pytest.mark.parametrize('sim', R.SIMS)
def test_knn_topk_small(sim, shrinkage, k, tile_cols):
    v, b, dense = small_truth(sim, shrinkage)
    idx, val, length = run_knn(small_matrix(), sim, k, shrinkage, tile_cols=tile_cols, **PARAMS[sim])
    R.check_kernel_lists(idx, val, length, v, b, k, what=f'{sim} s={shrinkage} k={k} tile={tile_cols}')
    assert length[17] == 0                                            # the empty row
    assert (dense > 0).sum(axis=1).max() > 100                        # k = 100 prunes, k = 256 does not
    if k >= 5:                                                        # the identical rows head each other's list unless beaten by index
        assert 101 in idx[40, :length[40]] and 40 in idx[101, :length[101]]
        if sim == 'jaccard' and shrinkage == 0.:
            assert val[40][list(idx[40]).index(101)] == 1.0 and idx[40, 0] == 101 and idx[101, 0] == 40


@pytest.mark.parametrize('n', [1, 2])
def test_knn_topk_one_and_two_rows(n):
    x = sp.csr_matrix(np.ones((n, 3), dtype=np.float32))
    idx, val, length = run_knn(x, 'jaccard', 4)
    if n == 1:
        assert length.tolist() == [0] and idx.tolist() == [[-1] * 4] and val.tolist() == [[0.] * 4]
    else:
        assert length.tolist() == [1, 1] and idx.tolist() == [[1, -1, -1, -1], [0, -1, -1, -1]] and val[:, 0].tolist() == [1., 1.]


def test_knn_topk_a_feature_every_row_has():
    rng = np.random.default_rng(5)
    d = rng.random((70, 20)) < 0.1
    d[:, 7] = True
    x = sp.csr_matrix(d.astype(np.float32))
    for k, tile in ((10, 64), (69, 64), (100, 0)):
        v, b = R.sparse_values_and_bound(x, 'cosine', 2.)
        idx, val, length = run_knn(x, 'cosine', k, 2., tile_cols=tile)
        assert (length == min(k, 69)).all()                           # every pair is a candidate
        R.check_kernel_lists(idx, val, length, v, b, k, what=f'common feature k={k}')


@pytest.mark.parametrize('sim', R.SIMS)
def test_knn_topk_identical_rows(sim):
    row = np.zeros(50, dtype=np.float32)
    row[[3, 8, 20, 21, 40, 41, 49]] = 1
    x = sp.csr_matrix(np.tile(row, (100, 1)))
    for k, tile in ((7, 64), (99, 64), (256, 0)):
        idx, val, length = run_knn(x, sim, k, 5., tile_cols=tile, **PARAMS[sim])
        for i in range(100):                                          # all values equal: exactly the ascending indices without self
            want = [j for j in range(100) if j != i][:k]
            assert idx[i, :length[i]].tolist() == want, f'{sim} k={k} row {i}'
        assert len(np.unique(val[:, 0])) == 1 and (val[:, :min(k, 99)] == val[0, 0]).all()


def test_knn_topk_heavy_contention_and_repeat():
    """512 x 3000 at density 0.5: counts in the hundreds, every counter hit by many waves at once; two runs agree in bits"""
    rng = np.random.default_rng(7)
    x = sp.csr_matrix((rng.random((512, 3000)) < 0.5).astype(np.float32))
    c = R.counts(x)
    assert c[~np.eye(512, dtype=bool)].min() > 300
    first = None
    for sim in ('jaccard', 'cosine'):
        v = R.values(x, sim, 5., c=c)
        b = R.value_bound(x, sim, 5., c=c, v=v)
        got = run_knn(x, sim, 100, 5.)
        R.check_kernel_lists(*got, v, b, 100, what=f'contention {sim}')
        first = first or got
    again = run_knn(x, 'jaccard', 100, 5.)
    for a, g in zip(first, again):
        assert np.array_equal(a.view(np.int32), g.view(np.int32))


def test_knn_topk_two_default_tiles():
    """33,000 x 20,000 with 4 entries per row: the default tile (32,768 counters) does not cover the rows, the lists are carried across"""
    rng = np.random.default_rng(9)
    n, m = 33000, 20000
    cols = np.argsort(rng.random((n, 40)), axis=1)[:, :4] + rng.integers(0, m - 40, size=(n, 1))
    x = sp.csr_matrix((np.ones(n * 4, dtype=np.float32), (np.repeat(np.arange(n), 4), cols.ravel())), shape=(n, m))
    assert x.nnz == 4 * n
    v, b = R.sparse_values_and_bound(x, 'cosine', 1.)
    assert v.nnz < 1_000_000
    n_cand = np.diff(v.indptr)
    beyond = np.asarray((v[:, 32768:] > 0).sum(axis=1)).ravel()
    assert ((n_cand > 5) & (beyond > 0) & (beyond < n_cand)).sum() > 100          # pruned rows with candidates in both tiles
    idx, val, length = run_knn(x, 'cosine', 5, 1.)
    R.check_kernel_lists(idx, val, length, v, b, 5, what='two tiles')


def test_knn_topk_row_range():
    x = small_matrix()
    v, b, _ = small_truth('tversky', 5.)
    full = run_knn(x, 'tversky', 5, 5., tile_cols=64, **PARAMS['tversky'])
    part = run_knn(x, 'tversky', 5, 5., tile_cols=64, rows=(40, 97), **PARAMS['tversky'])        # (run_knn checks the other rows' bits)
    for f, p in zip(full, part):
        assert np.array_equal(f[40:97].view(np.int32), p[40:97].view(np.int32))
    R.check_kernel_lists(*part, v, b, 5, rows=range(40, 97), what='row range')
    run_knn(x, 'tversky', 5, 5., rows=(33, 33), **PARAMS['tversky'])                              # an empty range writes nothing


def test_knn_topk_invalid_arguments():
    Sm = S()
    x = small_matrix()
    for kw, word in ((dict(k=0), 'k=0'), (dict(k=257), 'k=257'), (dict(k=5, shrinkage=-1.), 'shrinkage'), (dict(k=5, alpha=-.5), 'alpha'),
                     (dict(k=5, beta=-.5), 'alpha / beta'), (dict(k=5, tile_cols=50000), '160 KiB')):
        with pytest.raises(Sm.SibrarHipError, match='sbr_knn_topk.*' + word):
            run_knn(x, 'tversky', check=False, **kw)


def test_ops_knn_topk_in_deterministic_mode():
    Sm = S()
    feats = __import__('importlib').import_module(Sm.ops.__name__.rsplit('.', 1)[0] + '.features')
    x = small_matrix()
    csr = feats.DeviceCSR(x).to(DEV)
    v, b, _ = small_truth('cosine', 5.)
    prev = Sm.ops.set_deterministic(True)
    try:
        Sm.ops.nondeterministic_launches(reset=True)
        idx, val, length = Sm.ops.knn_topk(csr, 'cosine', 5, 5.)
        part = Sm.ops.knn_topk(csr, Sm.SimilarityFunctionEnum.cosine, 5, 5., rows=(10, 20), tile_cols=64)
        torch.cuda.synchronize()
        assert Sm.ops.nondeterministic_launches() == 0
    finally:
        Sm.ops.set_deterministic(prev)
    R.check_kernel_lists(idx.cpu().numpy(), val.cpu().numpy(), length.cpu().numpy(), v, b, 5, what='ops.knn_topk')
    assert torch.equal(part[0][10:20], idx[10:20]) and torch.equal(part[1][10:20], val[10:20]) and torch.equal(part[2][10:20], length[10:20])
    assert bool((part[0][:10] == -1).all()) and bool((part[2][20:] == 0).all())
    with pytest.raises(ValueError, match='0/1'):
        Sm.ops.knn_topk(feats.DeviceCSR(x * 2).to(DEV), 'cosine', 5)
    with pytest.raises(ValueError, match='unknown similarity'):
        Sm.ops.knn_topk(csr, 'dense_cosine', 5)


# ---- sbr_csr_rows_times_csr ----------------------------------------------------------------------------------------------------------
def _sparse(rng, shape, density, values):
    d = rng.random(shape) < density
    m = sp.csr_matrix(np.where(d, rng.standard_normal(shape) if values else 1., 0.).astype(np.float32))
    m.sort_indices()
    return m


@functools.lru_cache(maxsize=None)
def product_operands(x_values, y_values, wide):
    rng = np.random.default_rng(31 + 2 * x_values + y_values + 4 * wide)
    x = _sparse(rng, (40, 200), 0.45, x_values).tolil()        # rows of ~90 entries: more than one batch of 64
    x[5] = 0                                                    # an empty row
    x = sp.csr_matrix(x)
    x.eliminate_zeros()
    # narrow: rows of ~22 entries (scanned from their start); wide: rows of ~350 entries (entered by a lower bound)
    y = _sparse(rng, (200, 700 if wide else 150), 0.5 if wide else 0.15, y_values)
    return x, y


@pytest.mark.parametrize('tile_cols', [64, 0])
@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('y_values', [False, True])
@pytest.mark.parametrize('x_values', [False, True])
def test_csr_rows_times_csr(x_values, y_values, wide, tile_cols):
    x, y = product_operands(x_values, y_values, wide)
    n_cols = y.shape[1]
    rows = np.array([7, 5, 39, 0, 7, 7, 12, 5, 38, 1], dtype=np.int64)               # unsorted, with repeats, with the empty row
    xp, xi = _csr_dev(x)
    yp, yi = _csr_dev(y)
    xd = torch.from_numpy(x.data).to(DEV) if x_values else None
    yd = torch.from_numpy(y.data).to(DEV) if y_values else None
    xs, ys = x[rows].astype(np.float64), y.astype(np.float64)
    ref = np.asarray((xs @ ys).todense())
    mag = np.asarray((abs(xs) @ abs(ys)).todense())
    terms = np.asarray(((xs != 0).astype(np.float64) @ (ys != 0).astype(np.float64)).todense())
    outs = []
    for ld in (n_cols, n_cols + 7, n_cols):
        out = _Buf(len(rows), n_cols, ld=ld, off=1)
        call('sbr_csr_rows_times_csr', _p(xp), _p(xi), _p(xd), _p(_i64(rows)), len(rows), _p(yp), _p(yi), _p(yd), n_cols, tile_cols, out.ptr, ld,
             _L().stream())
        got = out.check_untouched(what=f'ld={ld}').contiguous()
        assert not bool(torch.isnan(got).any()), 'an element of the addressed rows was not written'
        outs.append(got)
    got = outs[0].double().numpy()
    if not x_values and not y_values:
        assert np.array_equal(got, ref)                                                # integer results are exact
    assert np.all(np.abs(got - ref) <= R.gamma(terms) * mag)
    assert np.all(got[terms == 0] == 0) and not np.signbit(got[terms == 0]).any()
    assert np.all(got[[1, 7]] == 0)                                                    # the empty row of X
    _assert_bits(outs[1], outs[0], 'ld')
    _assert_bits(outs[2], outs[0], 'repeat')


@functools.lru_cache(maxsize=None)
def ordered_product(n_cols, y_values):
    x, rows, y = R.ordered_product_operands(n_cols)
    if not y_values:
        y = abs(y).sign().astype(np.float32)
    return x, rows, y, R.csr_rows_times_csr_ordered(x, rows, y)


@pytest.mark.parametrize('tile_cols', [64, 0])
@pytest.mark.parametrize('y_values', [False, True])
@pytest.mark.parametrize('n_cols', [70, 134])
def test_csr_rows_times_csr_summation_order(n_cols, y_values, tile_cols):
    """Bit equality with the order oracle of knn_ref (exact: X holds powers of two). tile_cols = 64: strips of 16 columns, the last one
    of 6; X rows of 0, 1, 63, 64, 65 and 130 entries; Y rows of up to 129 entries at n_cols = 134 (scanned up to 128, entered by a
    lower bound above), which a Y of 70 columns cannot hold: there every row is scanned, with entries on both sides of the strip edges."""
    x, rows, y, ref = ordered_product(n_cols, y_values)
    xp, xi = _csr_dev(x)
    yp, yi = _csr_dev(y)
    xd = torch.from_numpy(x.data).to(DEV)
    yd = torch.from_numpy(y.data).to(DEV) if y_values else None
    out = _Buf(len(rows), n_cols, ld=n_cols + 3, off=1)
    call('sbr_csr_rows_times_csr', _p(xp), _p(xi), _p(xd), _p(_i64(rows)), len(rows), _p(yp), _p(yi), _p(yd), n_cols, tile_cols, out.ptr,
         n_cols + 3, _L().stream())
    _assert_bits(out.check_untouched().contiguous().cpu(), torch.from_numpy(ref), f'n_cols={n_cols} y_values={y_values} tile_cols={tile_cols}')


def test_ops_csr_rows_times_csr_all_rows_and_errors():
    Sm = S()
    feats = __import__('importlib').import_module(Sm.ops.__name__.rsplit('.', 1)[0] + '.features')
    x, y = product_operands(True, False, False)
    xd, yd = feats.DeviceCSR(x).to(DEV), feats.DeviceCSR(y).to(DEV)
    assert yd.data is None
    got = Sm.ops.csr_rows_times_csr(xd, None, yd).cpu().double().numpy()
    xs, ys = x.astype(np.float64), y.astype(np.float64)
    terms = np.asarray(((xs != 0).astype(np.float64) @ ys).todense())
    assert np.all(np.abs(got - np.asarray((xs @ ys).todense())) <= R.gamma(terms) * np.asarray((abs(xs) @ ys).todense()))
    picked = Sm.ops.csr_rows_times_csr((xd.indptr, xd.indices, xd.data, xd.shape), torch.tensor([3, 3, 0], device=DEV), yd, tile_cols=64)
    assert np.array_equal(picked.cpu().double().numpy(), got[[3, 3, 0]])
    with pytest.raises(ValueError, match='do not chain'):
        Sm.ops.csr_rows_times_csr(yd, None, yd)
    with pytest.raises(Sm.SibrarHipError, match='sbr_csr_rows_times_csr'):
        Sm.ops.csr_rows_times_csr(xd, None, yd, tile_cols=1 << 20)


# ---- the models --------------------------------------------------------------------------------------------------------------------
ARRAYS, CASES = R.load_g22()


def _model(case, **kw):
    Sm = S()
    return Sm.KNNAlgorithm.build_from_conf({'alg': case['alg'], 'k': case['k'], 'shrinkage': case['shrinkage'],
                                            'sim_func_params': {'sim_func_name': case['sim'], **case['params']}}, None)


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_models_meet_the_reference(case):
    inter = sp.csr_matrix(ARRAYS['inter'])
    m = _model(case).fit(inter)
    n_users, n_items = inter.shape
    pred = m.combine_user_item_representations(m.get_user_representations(torch.arange(n_users)), m.get_item_representations(torch.arange(n_items)))
    assert pred.shape == (n_users, n_items)
    p = case['params']
    R.check_case_against_fixture(case, ARRAYS, m.nbr_idx.cpu().numpy(), m.nbr_val.cpu().numpy(), m.nbr_len.cpu().numpy(), pred.cpu().numpy(),
                                 lambda v, c: R.value_bound(None, case['sim'], case['shrinkage'], p.get('alpha'), p.get('beta'), c, v))


@pytest.mark.parametrize('alg', ['uknn', 'iknn'])
def test_predict_is_the_gather_of_combine_and_survives_a_round_trip(alg, tmp_path):
    Sm = S()
    case = next(c for c in CASES if c['name'] == f'{alg}_jaccard_s5_k5')
    inter = sp.csr_matrix(ARRAYS['inter'])
    m = _model(case).fit(inter)
    rng = np.random.default_rng(3)
    u = torch.from_numpy(rng.integers(0, 50, size=16))
    i = torch.from_numpy(rng.integers(0, 40, size=(16, 9)))
    full = m.combine_user_item_representations(m.get_user_representations(u), m.get_item_representations(torch.arange(40)))
    got = m.predict(u, i)
    assert got.shape == (16, 9) and torch.equal(got, torch.gather(full, 1, i.to(DEV)))
    some = torch.tensor([31, 2, 2, 17])
    assert torch.equal(m.combine_user_item_representations(m.get_user_representations(u), m.get_item_representations(some)), full[:, some.to(DEV)])
    # S as CSR equals the lists
    indptr, indices, data, shape = m.similarity_csr()
    s = sp.csr_matrix((data.cpu().numpy(), indices.cpu().numpy(), indptr.cpu().numpy()), shape=shape).toarray()
    assert np.array_equal(s, R.lists_to_dense(m.nbr_idx.cpu().numpy(), m.nbr_val.cpu().numpy(), m.nbr_len.cpu().numpy()).astype(np.float32))
    m.save_model_to_path(str(tmp_path))
    back = _model(case)
    back.load_model_from_path(str(tmp_path), matrix=inter)
    assert torch.equal(back.predict(u, i), got)


@pytest.mark.parametrize('scorer', ['fp32', 'fp16_fused'])
@pytest.mark.parametrize('alg', ['uknn', 'iknn'])
def test_evaluate_recommender_algorithm(alg, scorer):
    """plumbing: the metrics are those of the stable top-k (tests/evalk_ref.py) of the model's own masked score rows"""
    Sm = S()
    ds = Sm.SyntheticDataset(300, 200, 4000, seed=6, n_negative_samples=3, holdout_per_user=1)
    m = Sm.ALGORITHMS[alg](Sm.SimilarityFunctionEnum.cosine, k=20, shrinkage=1.).fit(ds.user_sampling_matrix_train)
    view = ds.eval_view()
    ks = (1, 5, 10)
    ev = Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=ks, metrics=('ndcg', 'recall', 'precision')), dataset=view)
    loader = type('L', (), {'dataset': view, 'batch_size': 64})()
    kw = {} if scorer == 'fp32' else {'scorer': scorer}
    metrics, raw = Sm.evaluate_recommender_algorithm(m, loader, ev, DEV, return_raw=True, user_chunk=128, **kw)
    users = np.asarray(view.users_in_split)
    items = torch.as_tensor(np.asarray(view.items_in_split))
    rows = m.combine_user_item_representations(m.get_user_representations(torch.from_numpy(users)), m.get_item_representations(items))
    excl = sp.csr_matrix(view.exclude_data)
    excl.sort_indices()
    masked = E.mask_ref(rows.cpu(), users, (excl.indptr, excl.indices))
    assert bool((masked > 0).any())
    _, top = E.topk_ref(masked, max(ks))
    lab = sp.csr_matrix(view.user_sampling_matrix)[:, np.asarray(view.items_in_split)]
    lab.sort_indices()
    got = np.stack([np.stack([raw[f'{name}@{k}'] for k in ks]) for name in ('ndcg', 'recall', 'precision')])
    E.check_metrics(got, top, users, (lab.indptr, lab.indices), ks, what=f'{alg} {scorer}')
    assert metrics['ndcg@10'] == pytest.approx(float(got[0, 2].mean()), rel=1e-6) and metrics['ndcg@10'] > 0
