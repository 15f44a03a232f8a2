"""The hooks the four fit(matrix) models share (sibrar_amd.matrix_models) on the GPU: a 1-D item subset, a 2-D item matrix and predict are
selections of the same fp32 score rows, bit for bit, and the rows survive a move to the host and back. Each model is fitted once on the
50 x 40 matrix of its golden fixture (g22, g23; g24's matrix with an empty user and an empty item)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import ease_ref
import knn_ref
import p3alpha_ref
from hip_testutil import DEV, S

pytestmark = pytest.mark.gpu

ALGS = ['uknn', 'iknn', 'ease', 'p3alpha']
RNG = np.random.default_rng(19)
U = torch.from_numpy(RNG.integers(0, 50, size=16))
SUBSET = torch.from_numpy(RNG.permutation(40)[:9])
ITEMS = torch.from_numpy(RNG.integers(0, 40, size=(16, 9)))


@functools.lru_cache(maxsize=None)
def fitted(alg):
    """(the fitted model, its score rows of U over all items) — made once, never changed"""
    if alg in ('uknn', 'iknn'):
        arrays, cases = knn_ref.load_g22()
        case = next(c for c in cases if c['name'] == f'{alg}_jaccard_s5_k5')
        conf = {'alg': alg, 'k': case['k'], 'shrinkage': case['shrinkage'], 'sim_func_params': {'sim_func_name': case['sim'], **case['params']}}
        inter = arrays['inter']
    elif alg == 'ease':
        arrays, cases = ease_ref.load_g23()
        conf, inter = {'alg': alg, 'lam': cases[0]['lam']}, arrays['inter']
    else:
        arrays, cases = p3alpha_ref.load_g24()
        case = next(c for c in cases if c['matrix'] == 'inter_empty')
        conf, inter = {'alg': alg, 'alpha': case['alpha']}, arrays['inter_empty']
    assert inter.shape == (50, 40)
    m = S().ALGORITHMS[alg].build_from_conf(conf, None).fit(sp.csr_matrix(inter))
    full = _combine(m, U, torch.arange(40))
    assert full.dtype == torch.float32 and tuple(full.shape) == (16, 40) and bool((full != 0).any())
    return m, full


def _combine(m, u, items):
    return m.combine_user_item_representations(m.get_user_representations(u), m.get_item_representations(items))


@pytest.mark.parametrize('alg', ALGS)
def test_subsets_and_predict_are_selections_of_the_same_rows(alg):
    m, full = fitted(alg)
    assert isinstance(m, S().ResidentMatrixAlgorithm)
    assert torch.equal(_combine(m, U, SUBSET), full[:, SUBSET.to(DEV)])
    want = torch.gather(full, 1, ITEMS.to(DEV))
    assert torch.equal(_combine(m, U, ITEMS), want)
    got = m.predict(U, ITEMS)
    assert got.dtype == torch.float32 and not got.requires_grad and torch.equal(got, want)


@pytest.mark.parametrize('alg', ALGS)
def test_rows_survive_a_move_to_the_host_and_back(alg):
    m, full = fitted(alg)
    assert m.to('cpu').device == torch.device('cpu')
    assert m.to(DEV) is m and torch.equal(_combine(m, U, torch.arange(40)), full)
