"""UserKNN / ItemKNN without a GPU: the float64 restatement of tests/knn_ref.py against the g22 fixture recorded from the reference, and the
host side of sibrar_amd.knn — registry, constructor defaults, build_from_conf, the ValueErrors, the model.npz round trip, the header."""
import importlib
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import knn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def S():
    import sibrar_amd
    return sibrar_amd


ARRAYS, CASES = R.load_g22()


def test_g22_covers_the_cases():
    want = {f'{a}_{s}_s{sh}_k{k}' for a in ('uknn', 'iknn') for s in R.SIMS for sh in (0, 5) for k in (5, 60)}
    assert {c['name'] for c in CASES} == want
    assert ARRAYS['inter'].shape == (50, 40) and set(np.unique(ARRAYS['inter'])) == {0., 1.}
    for c in CASES:
        if c['k'] == 60:
            assert c['max_candidates'] < 60 and c['rows_tied_at_boundary'] == 0
        else:
            assert c['rows_tied_at_boundary'] <= 0.6 * c['rows']


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_restatement_meets_the_reference(case):
    ent = R.entity_matrix(case['alg'], ARRAYS['inter'])
    v64 = R.values(ent, case['sim'], case['shrinkage'], case['params'].get('alpha'), case['params'].get('beta'))
    idx, val, length = R.lists(v64, case['k'])
    pred = R.predict(case['alg'], R.lists_to_dense(idx, val, length), ARRAYS['inter'])
    # float64 against float64: the reference's other operation order only (1e-12 relative)
    compared = R.check_case_against_fixture(case, ARRAYS, idx, val, length, pred, lambda v, c: 1e-12 * v)
    assert compared >= 0.4 * case['rows']


def test_the_rule_rejects_a_wrong_neighbour():
    case = next(c for c in CASES if c['name'] == 'uknn_cosine_s0_k5')
    ent = R.entity_matrix('uknn', ARRAYS['inter'])
    v64 = R.values(ent, 'cosine')
    idx, val, length = R.lists(v64, 5)
    row = int(np.flatnonzero(~R.boundary_tied(v64, 5) & ((v64 > 0).sum(axis=1) > 5))[0])
    worse = np.flatnonzero(v64[row] > 0)
    worse = worse[np.argsort(v64[row, worse])][0]                      # the row's weakest candidate in place of its best
    idx[row, 0], val[row, 0] = worse, v64[row, worse]
    with pytest.raises(AssertionError):
        R.check_case_against_fixture(case, ARRAYS, idx, val, length, None, lambda v, c: 1e-12 * v)


@pytest.mark.parametrize('n_cols', [70, 134])
def test_ordered_product_oracle_is_exact_and_meets_float64(n_cols):
    x, rows, y = R.ordered_product_operands(n_cols)
    assert [x.indptr[r + 1] - x.indptr[r] for r in range(6)] == [0, 1, 63, 64, 65, 130] and len(set(rows.tolist())) < len(rows)
    want = {0, 5, 128, 129} if n_cols >= 130 else {0, 5, n_cols // 2, n_cols}
    assert set(np.diff(y.indptr).tolist()) == want and np.abs(y.data).max() <= 4
    assert set(np.log2(x.data).tolist()) <= set(range(-3, 4))
    # the precondition of exactness: no product of an X value and a Y value rounds, underflows or overflows in float32
    for v in np.unique(x.data):
        prod = v * y.data
        assert prod.dtype == np.float32 and np.array_equal(prod.astype(np.float64), float(v) * y.data.astype(np.float64))
        assert np.all(np.abs(prod) >= np.finfo(np.float32).tiny) and np.all(np.isfinite(prod))
    for yy in (y, abs(y).sign().astype(np.float32)):                                   # y_data given, and NULL (ones)
        got = R.csr_rows_times_csr_ordered(x, rows, yy).astype(np.float64)
        xs, ys = x[rows].astype(np.float64), yy.astype(np.float64)
        terms = np.asarray(((xs != 0).astype(np.float64) @ (ys != 0).astype(np.float64)).todense())
        assert np.all(np.abs(got - np.asarray((xs @ ys).todense())) <= R.gamma(terms) * np.asarray((abs(xs) @ abs(ys)).todense()))
        assert np.array_equal(got[1], np.zeros(n_cols)) and np.array_equal(got[2], got[6])   # the empty row; the repeated row


def test_ordered_product_oracle_is_order_sensitive():
    """one row, one column, terms 1, 2^-24, 2^-24: ascending (1 + 2^-24) + 2^-24 = 1 (two ties to even), descending 2^-23 + 1"""
    xv, yv = np.float32([1., 2. ** -3, 2. ** -3]), np.float32([1., 2. ** -21, 2. ** -21])
    fwd = R.csr_rows_times_csr_ordered(sp.csr_matrix(xv[None, :]), [0], sp.csr_matrix(yv[:, None]))
    rev = R.csr_rows_times_csr_ordered(sp.csr_matrix(xv[None, ::-1]), [0], sp.csr_matrix(yv[::-1, None]))
    assert fwd[0, 0] == np.float32(1.) and rev[0, 0] == np.float32(1. + 2. ** -23)
    assert fwd.view(np.int32)[0, 0] != rev.view(np.int32)[0, 0]
    assert abs(float(rev[0, 0]) - (1 + 2. ** -23)) <= R.gamma(3) * (1 + 2. ** -23)


def test_value_bound_is_the_stated_count():
    x = ARRAYS['inter']
    for sim, n_round in (('cosine', 4), ('jaccard', 1), ('sorensen_dice', 1), ('tversky', 5)):
        v = R.values(x, sim, 0., 0.7, 0.2)
        b = R.value_bound(x, sim, 0., 0.7, 0.2)
        assert np.allclose(b[v > 0] / v[v > 0], R.gamma(n_round), rtol=1e-12)
        b5 = R.value_bound(x, sim, 5., 0.7, 0.2)
        v5 = R.values(x, sim, 5., 0.7, 0.2)
        assert np.allclose(b5[v5 > 0] / v5[v5 > 0], R.gamma(n_round + 4), rtol=1e-12)
    v, b = R.values(x, 'asymmetric_cosine', 0., 0.3), R.value_bound(x, 'asymmetric_cosine', 0., 0.3)
    assert np.all(b[v > 0] / v[v > 0] >= R.gamma(66)) and np.all(b[v > 0] / v[v > 0] <= R.gamma(66 + 1.3 * np.log(50)))


def test_registry_and_defaults():
    Sm = S()
    assert Sm.ALGORITHMS['uknn'] is Sm.UserKNN and Sm.ALGORITHMS['iknn'] is Sm.ItemKNN
    assert [e.name for e in Sm.SimilarityFunctionEnum] == ['jaccard', 'cosine', 'dense_cosine', 'asymmetric_cosine', 'tversky', 'sorensen_dice']
    for cls, name in ((Sm.UserKNN, 'UserKNN'), (Sm.ItemKNN, 'ItemKNN')):
        m = cls()
        assert (m.sim_func_enum, m.k, m.shrinkage, m.name) == (Sm.SimilarityFunctionEnum.cosine, 100, 0., name)
        assert isinstance(m, Sm.KNNAlgorithm) and isinstance(m, Sm.SparseMatrixBasedRecommenderAlgorithm)
        assert m.eval() is m and m.train() is m
    m = Sm.ItemKNN(Sm.SimilarityFunctionEnum.tversky, 7, 2.5, alpha=0.7, beta=0.2)
    assert (m.k, m.shrinkage, m.alpha, m.beta) == (7, 2.5, 0.7, 0.2)
    with pytest.raises(KeyError):
        Sm.UserKNN(Sm.SimilarityFunctionEnum.asymmetric_cosine)          # alpha is required, as in the reference (kwargs['alpha'])


@pytest.mark.parametrize('alg,cls', [('uknn', 'UserKNN'), ('iknn', 'ItemKNN')])
def test_build_from_conf(alg, cls):
    Sm = S()
    m = Sm.KNNAlgorithm.build_from_conf({'alg': alg, 'k': 12, 'sim_func_params': {'sim_func_name': 'jaccard'}}, None)
    assert type(m) is getattr(Sm, cls) and (m.k, m.shrinkage, m.sim_func_enum.name) == (12, 0., 'jaccard')
    m = Sm.ALGORITHMS[alg].build_from_conf({'alg': alg, 'k': 3, 'shrinkage': 4., 'sim_func_params': {'sim_func_name': 'tversky', 'alpha': 0.5,
                                                                                                    'beta': 0.25}}, None)
    assert type(m) is getattr(Sm, cls) and (m.k, m.shrinkage, m.alpha, m.beta) == (3, 4., 0.5, 0.25)
    with pytest.raises(ValueError, match='ifknn'):
        Sm.KNNAlgorithm.build_from_conf({'alg': 'ifknn', 'k': 3, 'sim_func_params': {'sim_func_name': 'cosine'}}, None)
    with pytest.raises(ValueError, match='invalid model'):
        Sm.KNNAlgorithm.build_from_conf({'alg': 'ease', 'k': 3, 'sim_func_params': {'sim_func_name': 'cosine'}}, None)


def test_value_errors():
    Sm = S()
    with pytest.raises(ValueError, match='ifknn'):
        Sm.ItemKNN(Sm.SimilarityFunctionEnum.dense_cosine)
    for k in (0, -1, 257, 2.5):
        with pytest.raises(ValueError, match='k='):
            Sm.UserKNN(k=k)
    with pytest.raises(ValueError, match='shrinkage'):
        Sm.UserKNN(shrinkage=-1.)
    x = sp.csr_matrix(np.array([[1., 2.], [0., 1.]]))
    with pytest.raises(ValueError, match='0/1'):
        Sm.ItemKNN(device='cpu').fit(x)
    dup = sp.coo_matrix((np.ones(3), ([0, 0, 1], [1, 1, 0])), shape=(2, 2))      # a duplicate entry sums to 2
    with pytest.raises(ValueError, match='0/1'):
        Sm.UserKNN(device='cpu').fit(dup)


def test_model_npz_round_trip(tmp_path):
    Sm = S()
    idx = torch.tensor([[2, 1, -1], [0, -1, -1], [-1, -1, -1]], dtype=torch.int32)
    val = torch.tensor([[0.75, 0.5, 0.], [0.25, 0., 0.], [0., 0., 0.]], dtype=torch.float32)
    length = torch.tensor([2, 1, 0], dtype=torch.int32)
    m = Sm.ItemKNN(Sm.SimilarityFunctionEnum.jaccard, k=3, device='cpu')
    with pytest.raises(RuntimeError, match='fit'):
        m.save_model_to_path(str(tmp_path))
    m.nbr_idx, m.nbr_val, m.nbr_len = idx, val, length
    m.save_model_to_path(str(tmp_path))
    with np.load(tmp_path / 'model.npz', allow_pickle=False) as f:
        assert set(f.files) == {'nbr_idx', 'nbr_val', 'nbr_len', 'name', 'k', 'sim_func'}
        assert (str(f['name']), int(f['k']), str(f['sim_func'])) == ('ItemKNN', 3, 'jaccard')
    back = Sm.ItemKNN(Sm.SimilarityFunctionEnum.jaccard, k=3, device='cpu')
    back.load_model_from_path(str(tmp_path))
    assert torch.equal(back.nbr_idx, idx) and torch.equal(back.nbr_val, val) and torch.equal(back.nbr_len, length)
    assert back.nbr_idx.dtype == torch.int32 and back.nbr_val.dtype == torch.float32
    with pytest.raises(RuntimeError, match='attach'):
        back.predict(torch.tensor([0]), torch.tensor([[0]]))               # the file does not hold the interactions
    for other in (Sm.UserKNN(Sm.SimilarityFunctionEnum.jaccard, k=3), Sm.ItemKNN(k=3), Sm.ItemKNN(Sm.SimilarityFunctionEnum.jaccard, k=4)):
        with pytest.raises(ValueError, match='model.npz holds'):
            other.load_model_from_path(str(tmp_path))
    # the CSR form of the lists (host tensors: torch index ops only)
    knn = importlib.import_module(Sm.knn.__name__)
    indptr, indices, data, shape = knn._lists_to_csr(idx, val, length, False)
    assert (indptr.tolist(), indices.tolist(), data.tolist(), shape) == ([0, 2, 3, 3], [1, 2, 0], [0.5, 0.75, 0.25], (3, 3))
    indptr, indices, data, shape = knn._lists_to_csr(idx, val, length, True)
    assert (indptr.tolist(), indices.tolist(), data.tolist()) == ([0, 1, 2, 3], [1, 0, 0], [0.25, 0.5, 0.75])


def test_a_reference_model_file_is_refused(tmp_path):
    Sm = S()
    np.savez(tmp_path / 'model.npz', pred_mtx=np.zeros((2, 2)))
    with pytest.raises(ValueError, match='pred_mtx'):
        Sm.UserKNN().load_model_from_path(str(tmp_path))


def test_header_declares_both_symbols():
    lib = importlib.import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')
    protos = lib.parse_header()
    assert len(protos['sbr_knn_topk'][1]) == 18 and protos['sbr_knn_topk'][2][-4:] == ['nbr_idx', 'nbr_val', 'nbr_len', 'stream']
    assert len(protos['sbr_csr_rows_times_csr'][1]) == 13 and protos['sbr_csr_rows_times_csr'][2][3] == 'rows'
    text = open(os.path.join(ROOT, 'include', 'sibrar_hip.h')).read()
    assert 'utilities/similarities.py:18-130' in text and 'knn_algs.py:116' in text and 'knn_algs.py:96' in text
