"""ItemFeatureKNN without a GPU: the float64 restatement of tests/ifknn_ref.py against the g25 fixture recorded from the reference, and the
host side of sibrar_amd.knn — registry, constructor defaults, build_from_conf, the ValueErrors, the header."""
import importlib
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import ifknn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS, CASES = R.load_g25()


def S():
    import sibrar_amd
    return sibrar_amd


def test_g25_covers_the_cases():
    want = {f'ifknn_{w}_s{sh}_k{k}' for w, shs in (('signed', (0,)), ('abs', (0, 5))) for sh in shs for k in (5, 60)}
    assert {c['name'] for c in CASES} == want
    assert ARRAYS['inter'].shape == (50, 40) and ARRAYS['features'].shape == (40, 24)
    f = ARRAYS['features']
    assert not f[7].any() and np.array_equal(f[31], f[12]) and (f < 0).any()
    for c in CASES:
        assert R.candidates_are_precision_free(R.case_features(c, ARRAYS))
        if c['k'] == 60:
            assert c['max_candidates'] == 39 and c['rows_tied_at_boundary'] == 0
        else:
            assert c['rows_tied_at_boundary'] <= 0.1 * c['rows']
    assert next(c for c in CASES if c['name'] == 'ifknn_signed_s0_k60')['min_value'] < -0.5       # negative values are kept


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_restatement_meets_the_reference(case):
    v64, cand = R.values(R.case_features(case, ARRAYS), case['shrinkage'])
    idx, val, length = R.lists(v64, cand, case['k'])
    assert length[7] == 0 and (length[np.arange(40) != 7] == min(case['k'], 39)).all()
    if case['k'] == 60:
        assert all(i in idx[i, :39] for i in range(40) if i != 7)                               # the explicit self 0 is kept
    pred = R.predict(R.lists_to_dense(idx, val, length), ARRAYS['inter'])
    compared = R.check_case_against_fixture(case, ARRAYS, idx, val, length, pred, fp32=False)
    assert compared == case['rows'] - case['rows_tied_at_boundary'] >= 0.9 * case['rows']


def test_the_rule_rejects_a_wrong_neighbour():
    case = next(c for c in CASES if c['name'] == 'ifknn_signed_s0_k5')
    v64, cand = R.values(ARRAYS['features'])
    idx, val, length = R.lists(v64, cand, 5)
    row = int(np.flatnonzero(~R.boundary_tied(v64, cand, 5) & (cand.sum(axis=1) > 5))[0])
    worst = np.flatnonzero(cand[row])
    worst = worst[np.argsort(v64[row, worst])][0]
    idx[row, 0], val[row, 0] = worst, v64[row, worst]
    with pytest.raises(AssertionError):
        R.check_case_against_fixture(case, ARRAYS, idx, val, length, None, fp32=False)


def test_exact_restatement_agrees_with_float64_on_integers():
    rng = np.random.default_rng(5)
    f = rng.integers(-4, 5, (30, 7)).astype(np.float32)
    f[3] = 0
    f[9] = -f[4]
    idx, val, length = R.lists_f32_exact(f, 8, 2.5)
    v64, cand = R.values(f, 2.5)
    i64, _, l64 = R.lists(v64, cand, 8)
    assert np.array_equal(length, l64) and length[3] == 0
    tied = R.boundary_tied(v64, cand, 8)
    for i in np.flatnonzero(~tied):
        assert set(idx[i, :length[i]].tolist()) == set(i64[i, :l64[i]].tolist())
    assert np.all(np.abs(val - v64[np.arange(30)[:, None], np.maximum(idx, 0)] * (idx >= 0)) <= 1e-5)


def test_bound_is_small_and_zero_on_the_diagonal():
    f = np.random.default_rng(1).normal(size=(20, 24)).astype(np.float32)
    b = R.value_bound(f)
    assert np.all(np.diag(b) == 0) and 0 < b.max() < 24 * 4 * R.U32 * 10
    b5 = R.value_bound(np.abs(f), 5.)
    assert np.all(b5 >= 0) and b5.max() < 1e-4
    with pytest.raises(AssertionError):
        R.value_bound(f, 5.)


# ---- the host side ------------------------------------------------------------------------------------------------------------------------
def test_registry_and_defaults():
    Sm = S()
    assert Sm.ALGORITHMS['ifknn'] is Sm.ItemFeatureKNN and issubclass(Sm.ItemFeatureKNN, Sm.KNNAlgorithm)
    assert issubclass(Sm.ItemFeatureKNN, Sm.ResidentMatrixAlgorithm)
    m = Sm.ItemFeatureKNN()
    assert (m.sim_func_enum, m.k, m.shrinkage, m.name, m.ENTITY) == (Sm.SimilarityFunctionEnum.dense_cosine, 100, 0., 'ItemFeatureKNN', 'item')
    assert Sm.ItemFeatureKNN('dense_cosine', k=7).k == 7


def test_build_from_conf():
    Sm = S()
    m = Sm.KNNAlgorithm.build_from_conf({'alg': 'ifknn', 'k': 3, 'shrinkage': 4., 'sim_func_params': {'sim_func_name': 'dense_cosine'}}, None)
    assert isinstance(m, Sm.ItemFeatureKNN) and (m.k, m.shrinkage) == (3, 4.)
    m = Sm.ALGORITHMS['ifknn'].build_from_conf({'alg': 'ifknn', 'k': 9, 'sim_func_params': {'sim_func_name': 'dense_cosine'}}, None)
    assert isinstance(m, Sm.ItemFeatureKNN) and (m.k, m.shrinkage) == (9, 0.)
    with pytest.raises(ValueError, match='ifknn.*dense_cosine'):
        Sm.KNNAlgorithm.build_from_conf({'alg': 'ifknn', 'k': 3, 'sim_func_params': {'sim_func_name': 'jaccard'}}, None)


def test_refusals():
    Sm = S()
    E = Sm.SimilarityFunctionEnum
    for sim in (E.cosine, E.jaccard, E.sorensen_dice, 'cosine'):
        with pytest.raises(ValueError, match='ifknn.*dense_cosine'):
            Sm.ItemFeatureKNN(sim)
    for cls in (Sm.ItemKNN, Sm.UserKNN):
        with pytest.raises(ValueError, match='ifknn') as e:
            cls(E.dense_cosine)
        assert 'does not provide' not in str(e.value)
    for k in (0, 257, 2.5):
        with pytest.raises(ValueError, match='k='):
            Sm.ItemFeatureKNN(k=k)
    with pytest.raises(ValueError, match='shrinkage'):
        Sm.ItemFeatureKNN(shrinkage=-1.)
    assert Sm.ops.KNN_SIM_CODES.get('dense_cosine') is None


def test_fit_refusals_before_any_kernel():
    """what fit refuses on the host: a non-binary matrix, a missing feature matrix, a wrong row count, entries that are not finite, shrinkage
    with negative features (device 'cpu': none of these reaches a kernel)"""
    Sm = S()
    inter = sp.csr_matrix((ARRAYS['inter'] != 0).astype(np.float32))
    f = ARRAYS['features']
    m = Sm.ItemFeatureKNN(k=5, device='cpu')
    with pytest.raises(ValueError, match='0/1'):
        m.fit(inter * 2, f)
    with pytest.raises(ValueError, match='feature_matrix'):
        m.fit(inter)
    with pytest.raises(ValueError, match='feature_matrix'):
        m.fit(inter, f[:39])
    with pytest.raises(ValueError, match='feature_matrix'):
        m.fit(inter, f[:, 0])
    for bad in (np.nan, np.inf):
        g = f.copy()
        g[3, 2] = bad
        with pytest.raises(ValueError, match='not finite'):
            m.fit(inter, g)
        with pytest.raises(ValueError, match='not finite'):
            m.fit(inter, torch.from_numpy(g))
    with pytest.raises(ValueError, match='not finite'):
        m.fit(inter, f * 1e300)                                                                 # inf after the cast to float32
    with pytest.raises(ValueError, match='pole'):
        Sm.ItemFeatureKNN(k=5, shrinkage=5., device='cpu').fit(inter, sp.csr_matrix(f))
    assert m.nbr_idx is None
    with pytest.raises(RuntimeError, match='fit'):
        m.similarity_csr()


def test_ops_refusals_before_any_kernel():
    ops = S().ops
    f = torch.zeros(4, 3)
    for k in (0, 257, 1.5):
        with pytest.raises(ValueError, match='k='):
            ops.dense_knn_topk(f, k)
    with pytest.raises(ValueError, match='shrinkage'):
        ops.dense_knn_topk(f, 2, -1.)
    with pytest.raises(ValueError, match="dense_cosine|unknown similarity"):
        ops.knn_topk(None, 'dense_cosine', 3)


def test_header_declares_the_entries():
    lib = importlib.import_module('sibrar---single-branch-recommender_amd._lib')
    protos = lib.parse_header()
    assert protos['sbr_dense_knn_topk'][2] == ['F', 'norms', 'n', 'd', 'ld', 'r0', 'r1', 'shrinkage', 'k', 'nbr_idx', 'nbr_val', 'nbr_len', 'stream']
    assert protos['sbr_row_norms_f32'][2] == ['F', 'n', 'd', 'ld', 'norms', 'stream']
    text = open(os.path.join(ROOT, 'sibrar---single-branch-recommender_amd', 'csrc', 'Makefile')).read()
    assert 'dense_knn.hip' in text
