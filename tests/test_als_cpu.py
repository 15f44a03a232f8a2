"""ALS without a GPU: the float64 restatement of tests/als_ref.py against the minimiser of the full confidence-weighted least-squares
problem and its descent, the fp32 yardstick against the restatement, and the host side of sibrar_amd.als — registry, constructor,
build_from_conf, model.npz, the header and the library's exports."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import als_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = {'alg': 'als', 'alpha': 40, 'factors': 64, 'regularization': 0.01, 'n_iterations': 3, 'use_gpu': True}


def S():
    import sibrar_amd
    return sibrar_amd


def _small(weighted):
    rng = np.random.default_rng(5)
    d = (rng.random((6, 5)) < 0.5).astype(np.float64)
    if weighted:
        d *= rng.integers(1, 6, size=d.shape)
    d[4] = 0                                                                       # an empty row
    return sp.csr_matrix(d), rng.normal(size=(5, 3)) / 3


@pytest.mark.parametrize('weighted', [False, True])
def test_half_sweep_is_the_minimiser_of_the_weighted_least_squares_problem(weighted):
    """row by row: min_x sum_i c_i (p_i - x . y_i)^2 + reg ||x||^2 over ALL items, as a dense lstsq problem"""
    x, y = _small(weighted)
    alpha, reg = 40.0, 0.01
    got = R.half_sweep64(x, y, alpha, reg)
    d = np.asarray(x.todense())
    for r in range(6):
        c = np.where(d[r] != 0, alpha * d[r], 1.0)
        p = (d[r] != 0).astype(np.float64)
        lhs = np.vstack([np.sqrt(c)[:, None] * y, np.sqrt(reg) * np.eye(3)])
        rhs = np.concatenate([np.sqrt(c) * p, np.zeros(3)])
        want = np.linalg.lstsq(lhs, rhs, rcond=None)[0]
        assert np.abs(got[r] - want).max() <= 1e-10, f'row {r}'
    assert not got[4].any()


def test_loss_is_non_increasing_over_six_half_sweeps():
    x = R.world(30, 20, 0.2, seed=1, weighted=True)
    u0, i0 = R.uniform_factors(30, 4, 1), R.uniform_factors(20, 4, 2)
    trace = [R.loss64(x, u0, i0, 40, 0.01)]
    R.fit64(x, u0, i0, 40, 0.01, 3, trace)
    assert len(trace) == 7
    for a, b in zip(trace, trace[1:]):
        assert b <= a * (1 + 1e-12), trace


def test_the_yardstick_meets_the_restatement():
    x = R.world(40, 30, 0.2, seed=2)
    y = R.uniform_factors(30, 7, 3)
    g = R.gram32(y, 0.01)
    assert g.dtype == np.float32 and np.abs(g - R.gram64(y, 0.01)).max() <= 2 * 30 * R.EPS * np.abs(R.gram64(y, 0.01)).max()
    got = R.half_sweep32(x, y, 40, g)
    assert got.dtype == np.float32 and not got[1].any()
    be = R.backward_error(x, y, g, 40, got)
    print(f'yardstick backward error 40x30 f=7: {be:.3e}')
    assert be <= 7 * R.EPS * 8                                                     # the textbook f * eps with room for the assembly
    ref = R.half_sweep64(x, y, 40, 0.01, g=g)
    assert np.abs(got - ref).max() <= 1e-3 * np.abs(ref).max()


def test_registry_constructor_and_conf():
    Sm = S()
    cls = Sm.AlternatingLeastSquare
    assert Sm.ALGORITHMS['als'] is cls and issubclass(cls, Sm.SparseMatrixBasedRecommenderAlgorithm) and issubclass(cls, Sm.FactorModel)
    m = cls.build_from_conf(CONF, None)
    assert type(m) is cls and (m.name, m.alpha, m.factors, m.regularization, m.n_iterations, m.use_gpu) == ('AlternatingLeastSquare', 40, 64,
                                                                                                          0.01, 3, True)
    assert m.users_factors is None and m.items_factors is None and m.device == torch.device('cuda') and m.random_state == 0
    assert m.eval() is m and m.train() is m
    m = cls(2, 128, 0.1, 1, device='cpu', random_state=7)
    assert m.device == torch.device('cpu') and m.random_state == 7 and m.to('cpu') is m
    u, i = m.initial_factors(5, 4)
    rng = np.random.RandomState(7)
    assert np.array_equal(u, rng.uniform(-0.5 / 128, 0.5 / 128, size=(5, 128)).astype(np.float32))
    assert np.array_equal(i, rng.uniform(-0.5 / 128, 0.5 / 128, size=(4, 128)).astype(np.float32)) and i.dtype == np.float32
    for key in ('alpha', 'factors', 'regularization', 'n_iterations', 'use_gpu'):
        with pytest.raises(KeyError):
            cls.build_from_conf({k: v for k, v in CONF.items() if k != key}, None)
    mod = importlib.import_module(cls.__module__)
    for text in ('conjugate', 'use_gpu=False', 'fp32'):
        assert text in mod.__doc__                                                 # the deliberate differences are stated


def test_constructor_refusals():
    cls = S().AlternatingLeastSquare
    with pytest.raises(ValueError, match='no CPU fallback'):
        cls(40, 64, 0.01, 3, use_gpu=False)
    with pytest.raises(ValueError, match='no CPU fallback'):
        cls.build_from_conf(dict(CONF, use_gpu=False))
    for factors in (129, 0, -3, 2.5):
        with pytest.raises(ValueError, match='factors'):
            cls(40, factors, 0.01, 3)
    for alpha in (0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='alpha'):
            cls(alpha, 64, 0.01, 3)
    for reg in (0, -0.01, float('inf')):
        with pytest.raises(ValueError, match='regularization'):
            cls(40, 64, reg, 3)
    with pytest.raises(ValueError, match='n_iterations'):
        cls(40, 64, 0.01, -1)


def test_value_and_state_errors(tmp_path):
    cls = S().AlternatingLeastSquare
    m = cls(40, 4, 0.01, 1, device='cpu')
    with pytest.raises(ValueError, match='negative'):
        m.fit(sp.csr_matrix(np.array([[1., -2.], [0., 1.]])))
    with pytest.raises(RuntimeError, match='fit'):
        m.save_model_to_path(str(tmp_path))
    with pytest.raises(RuntimeError, match='fit'):
        m.predict(torch.tensor([0]), torch.tensor([[0]]))
    with pytest.raises(RuntimeError, match='fit'):
        m.get_user_representations(torch.tensor([0]))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.fit(sp.csr_matrix(np.array([[1., 3.], [0., 2.]])))                       # weighted data gets as far as the first kernel
    zero = cls(40, 4, 0.01, 0, device='cpu', random_state=3).fit(sp.csr_matrix(np.eye(3)))      # no sweep: the initial factors
    u, i = zero.initial_factors(3, 3)
    assert np.array_equal(zero.users_factors.numpy(), u) and np.array_equal(zero.items_factors.numpy(), i)
    assert torch.equal(zero.get_item_representations(torch.tensor([2, 0])), zero.items_factors[[2, 0]])
    assert torch.is_tensor(zero.get_user_representations(torch.tensor([1])))


def test_model_npz(tmp_path):
    cls = S().AlternatingLeastSquare
    m = cls(40, 3, 0.01, 1, device='cpu')
    m.users_factors, m.items_factors = torch.arange(12.).view(4, 3), torch.arange(6.).view(2, 3) / 4
    m.save_model_to_path(str(tmp_path))
    with np.load(tmp_path / 'model.npz', allow_pickle=False) as f:
        assert set(f.files) == {'users_factors', 'items_factors', 'name'} and str(f['name']) == 'AlternatingLeastSquare'
    back = cls(40, 3, 0.01, 1, device='cpu')
    back.load_model_from_path(str(tmp_path))
    assert torch.equal(back.users_factors, m.users_factors) and torch.equal(back.items_factors, m.items_factors)
    assert back.users_factors.dtype == torch.float32
    # a file written the reference's way (algorithms/mf_algs.py:127-130): float64 here, no name
    np.savez(tmp_path / 'model.npz', users_factors=np.ones((4, 3)), items_factors=np.full((2, 3), 0.5))
    back.load_model_from_path(str(tmp_path))
    assert back.users_factors.dtype == torch.float32 and torch.equal(back.items_factors, torch.full((2, 3), 0.5))
    np.savez(tmp_path / 'model.npz', users_factors=np.ones((4, 3)), items_factors=np.ones((2, 3)), name=np.array('EASE'))
    with pytest.raises(ValueError, match='holds a EASE'):
        back.load_model_from_path(str(tmp_path))
    np.savez(tmp_path / 'model.npz', users_factors=np.ones((4, 3)), items_factors=np.ones((2, 4)))
    with pytest.raises(ValueError, match='do not belong together'):
        back.load_model_from_path(str(tmp_path))
    assert torch.equal(back.items_factors, torch.full((2, 3), 0.5))                 # a refused file leaves the model as it is
    for fields in ({'pred_mtx': np.zeros((2, 2))}, {'pred_mtx': sp.csr_matrix(np.eye(2))}, {'B': np.zeros((2, 2)), 'name': np.array('EASE')},
                   {'users_factors': np.ones((4, 3)), 'items_factors': np.ones((2, 3)), 'pred_mtx': np.zeros((2, 2))}):
        np.savez(tmp_path / 'model.npz', **fields)
        with pytest.raises(ValueError, match='pred_mtx'):
            back.load_model_from_path(str(tmp_path))


def test_ops_refuse_host_and_wrong_operands():
    Sm = S()
    feats = importlib.import_module(Sm.ops.__name__.rsplit('.', 1)[0] + '.features')
    csr = feats.DeviceCSR(sp.csr_matrix(np.eye(3)))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Sm.ops.als_gram(torch.zeros(3, 4), 0.1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Sm.ops.als_solve_rows(csr, torch.zeros(3, 4), torch.eye(4), 40.)


def test_header_declares_and_library_exports_the_entry_points():
    lib = importlib.import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')
    protos = lib.parse_header()
    assert protos['sbr_als_gram_f32'][2] == ['Y', 'n_y', 'ldy', 'f', 'reg', 'G', 'ldg', 'workspace', 'workspace_bytes', 'stream']
    assert protos['sbr_als_gram_f32_workspace'][2] == ['n_y', 'f'] and protos['sbr_als_gram_f32_workspace'][0] is ctypes.c_long
    assert protos['sbr_als_solve_rows_f32'][2] == ['indptr', 'indices', 'data', 'r0', 'r1', 'Y', 'n_y', 'ldy', 'f', 'G', 'alpha', 'X', 'ldx',
                                                   'info', 'stream']
    assert protos['sbr_als_solve_rows_f32'][1][3] is ctypes.c_long and protos['sbr_als_solve_rows_f32'][1][10] is ctypes.c_float
    text = open(os.path.join(ROOT, 'include', 'sibrar_hip.h')).read()
    assert 'mf_algs.py:69-142' in text and text.count('New (additive to ABI 4)') >= 3 and 'ascending CSR order' in text
    assert 'als.hip' in open(os.path.join(os.path.dirname(lib.LIB_PATH), '..', 'csrc', 'Makefile')).read()
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name in ('sbr_als_gram_f32', 'sbr_als_gram_f32_workspace', 'sbr_als_solve_rows_f32'):
        assert hasattr(handle, name), name
    assert handle.sbr_abi_version() == 4
    # the argument checks come before anything touches the device: host arithmetic only
    handle.sbr_last_error.restype = ctypes.c_char_p
    L = lib.lib()
    assert L.sbr_als_gram_f32_workspace(1000, 128) == 2 * 128 * 128 * 4 and L.sbr_als_gram_f32_workspace(0, 5) == 0
    assert L.sbr_als_gram_f32_workspace(512, 3) == 36 and L.sbr_als_gram_f32_workspace(513, 3) == 72
    solve, gram = L.sbr_als_solve_rows_f32, L.sbr_als_gram_f32
    for args, word in (((None, None, None, 0, 5, None, 4, 129, 129, None, 40., None, 129, None, None), b'f=129'),
                       ((None, None, None, 0, 5, None, 4, 8, 8, None, 0., None, 8, None, None), b'alpha'),
                       ((None, None, None, 0, 5, None, 4, 8, 8, None, float('inf'), None, 8, None, None), b'alpha'),
                       ((None, None, None, 0, 5, None, 4, 8, 8, None, 40., None, 7, None, None), b'leading dimension'),
                       ((None, None, None, 0, 5, None, 4, 7, 8, None, 40., None, 8, None, None), b'leading dimension'),
                       ((None, None, None, 5, 4, None, 4, 8, 8, None, 40., None, 8, None, None), b'row range'),
                       ((None, None, None, -1, 4, None, 4, 8, 8, None, 40., None, 8, None, None), b'row range'),
                       ((None, None, None, 0, 5, None, 4, 8, 8, None, 40., None, 8, None, None), b'null operand')):
        assert solve(*args) != 0 and word in handle.sbr_last_error() and b'sbr_als_solve_rows_f32' in handle.sbr_last_error(), word
    assert solve(None, None, None, 3, 3, None, 4, 8, 8, None, 40., None, 8, None, None) == 0          # an empty range returns at once
    for args, word in (((None, 4, 0, 0, 0.1, None, 0, None, 0, None), b'f=0'),
                       ((None, 4, 8, 8, 0., None, 8, None, 0, None), b'reg'),
                       ((None, 4, 8, 8, float('nan'), None, 8, None, 0, None), b'reg'),
                       ((None, 4, 7, 8, 0.1, None, 8, None, 0, None), b'leading dimension'),
                       ((None, 4, 8, 8, 0.1, None, 8, None, 0, None), b'null operand')):
        assert gram(*args) != 0 and word in handle.sbr_last_error() and b'sbr_als_gram_f32' in handle.sbr_last_error(), word
