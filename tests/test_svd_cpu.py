"""SVD without a GPU: the fp32 yardstick of tests/svd_ref.py against the float64 truncated SVD on the gapped worlds (whose gap is asserted
here, from the regenerated matrix), the restated Jacobi's pair ordering and convergence, and the host side of sibrar_amd.svd — registry,
constructor, build_from_conf, initial_block, the refusals, model.npz, the header and the library's exports."""
import ctypes
import functools
import importlib
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import svd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def S():
    import sibrar_amd
    return sibrar_amd


@functools.lru_cache(maxsize=None)
def world(name):
    x = R.planted(*R.WORLDS[name])
    return x, R.svd64(x)[1]


@pytest.mark.parametrize('name', list(R.WORLDS))
def test_the_yardstick_reproduces_the_float64_truncated_scores(name):
    """recorded with OpenBLAS's LAPACK (oversample 28, tol 2e-6, RandomState(0)): 130x90/g5 7 iterations, scores within 3.6e-07 of the
    largest score; 300x200/g8 8 iterations, 9.5e-07; 700x260/g16 14 iterations, 2.1e-06; V^T V - I 2.2e-07 to 5.9e-07"""
    x, s = world(name)
    g = R.WORLDS[name][2]
    print(f'{name}: s_g {s[g - 1]:.2f} s_g+1 {s[g]:.2f}')
    assert s[g - 1] >= 1.3 * s[g], 'the planted world lost its spectral gap'
    b = min(g + 28, *x.shape)
    v0 = np.random.RandomState(0).standard_normal(size=(x.shape[1], b)).astype(np.float32)
    u, v, sv, iters, history = R.fit32(x, v0, g, 60, 2e-6)
    p64 = R.truncated64(x, g)
    dev = np.abs(u.astype(np.float64) @ v.astype(np.float64).T - p64).max() / np.abs(p64).max()
    orth = np.abs(v.astype(np.float64).T @ v.astype(np.float64) - np.eye(g)).max()
    print(f'{name}: fit32 {iters} iterations, residual {history[-1] / sv[0]:.2e} s_0, score deviation {dev:.2e}, V^T V - I {orth:.2e}')
    assert iters < 60 and history[-1] <= 2e-6 * sv[0]
    assert dev <= 1e-5 and orth <= 1e-5 and np.abs(sv - s[:g]).max() <= 1e-5 * s[0]


@pytest.mark.parametrize('n', [1, 2, 3, 7, 64, 65])
def test_round_robin_meets_every_pair_once_per_sweep(n):
    steps = R.round_robin(n)
    N = n + (n & 1)
    assert len(steps) == N - 1 and all(len(st) == N // 2 for st in steps)
    for st in steps:
        assert sorted(i for pq in st for i in pq) == list(range(N))               # disjoint: every index once per step (N - 1: the bye)
    met = [pq for st in steps for pq in st]
    assert len(set(met)) == len(met) == N * (N - 1) // 2 and all(p < q for p, q in met)


@pytest.mark.parametrize('n', [3, 7, 33])
def test_the_restated_jacobi_converges_and_decomposes(n):
    for name, a in R.eig_inputs(n).items():
        lam, w, sweeps, converged = R.jacobi32(a)
        res, orth = R.eig_figures(a, lam, w)
        print(f'jacobi32 n={n} {name}: {sweeps} sweeps, residual {res:.2e}, orthogonality {orth:.2e}')
        assert converged and sweeps < R.MAX_SWEEPS and bool((np.diff(lam) <= 0).all())
        assert res <= 64 * n * R.EPS and orth <= 64 * n * R.EPS                    # the textbook n * eps with room: this pins the restatement
        assert bool((w[np.abs(w).argmax(axis=0), np.arange(n)] > 0).all())


def test_registry_constructor_and_conf():
    Sm = S()
    cls = Sm.SVDAlgorithm
    assert Sm.ALGORITHMS['svd'] is cls and issubclass(cls, Sm.FactorModel) and issubclass(cls, Sm.SparseMatrixBasedRecommenderAlgorithm)
    m = cls.build_from_conf({'alg': 'svd', 'n_factors': 64}, None)
    assert type(m) is cls and (m.name, m.factors, m.oversample, m.random_state) == ('SVDAlgorithm', 64, 28, 0)
    assert m.n_iterations == 100 and m.tol == 1e-5 and m.device == torch.device('cuda')
    assert m.users_factors is None and m.items_factors is None and m.singular_values is None and m.n_iterations_run is None
    assert m.eval() is m and m.train() is m
    assert cls().factors == 100 and cls().oversample == 28 and cls(120).oversample == 8 and cls(128).oversample == 0
    with pytest.raises(KeyError):
        cls.build_from_conf({'alg': 'svd'}, None)
    m = cls(5, device='cpu', random_state=7, oversample=3, n_iterations=9, tol=1e-4)
    assert (m.device, m.random_state, m.oversample, m.n_iterations, m.tol) == (torch.device('cpu'), 7, 3, 9, 1e-4) and m.to('cpu') is m
    v0 = m.initial_block(11, 8)
    assert v0.dtype == np.float32 and np.array_equal(v0, np.random.RandomState(7).standard_normal(size=(11, 8)).astype(np.float32))
    mod = importlib.import_module(cls.__module__)
    for text in ('descending', 'sign', 'ARPACK', 'factors <= 128', 'fp32'):
        assert text in mod.__doc__                                                 # the deliberate differences are stated
    assert Sm.ops.SVD_MAX_BLOCK == 128


def test_refusals(tmp_path):
    cls = S().SVDAlgorithm
    for factors in (129, 0, -3, 2.5):
        with pytest.raises(ValueError, match='factors'):
            cls(factors)
    with pytest.raises(ValueError, match='n_iterations'):
        cls(4, n_iterations=-1)
    with pytest.raises(ValueError, match='oversample'):
        cls(4, oversample=1.5)
    with pytest.raises(ValueError, match='tol'):
        cls(4, tol=float('nan'))
    m = cls(4, device='cpu')
    with pytest.raises(ValueError, match=r'factors \(4\) exceeds min\(n_users, n_items\) = 3'):
        m.fit(sp.csr_matrix(np.eye(3)))
    for bad in (float('nan'), float('inf')):
        d = np.eye(5)
        d[2, 3] = bad
        with pytest.raises(ValueError, match='non-finite'):
            m.fit(sp.csr_matrix(d))
    with pytest.raises(RuntimeError, match='fit'):
        m.save_model_to_path(str(tmp_path))
    with pytest.raises(RuntimeError, match='fit'):
        m.predict(torch.tensor([0]), torch.tensor([[0]]))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.fit(sp.csr_matrix(-np.eye(4) * 2.5))                                     # any finite values get as far as the first kernel


def test_model_npz(tmp_path):
    Sm = S()
    cls = Sm.SVDAlgorithm
    m = cls(3, device='cpu')
    m.users_factors, m.items_factors = torch.arange(12.).view(4, 3), torch.arange(6.).view(2, 3) / 4
    m.save_model_to_path(str(tmp_path))
    with np.load(tmp_path / 'model.npz', allow_pickle=False) as f:
        assert set(f.files) == {'users_factors', 'items_factors', 'name'} and str(f['name']) == 'SVDAlgorithm'
    back = cls(3, device='cpu')
    back.load_model_from_path(str(tmp_path))
    assert torch.equal(back.users_factors, m.users_factors) and torch.equal(back.items_factors, m.items_factors)
    u, i = torch.tensor([3, 0]), torch.tensor([[1, 0], [0, 0]])
    assert torch.equal(back.get_user_representations(u), m.users_factors[u]) and torch.equal(back.get_item_representations(i[0]), m.items_factors[i[0]])
    # a file written the reference's way (algorithms/mf_algs.py:52-55): float64, no name
    np.savez(tmp_path / 'model.npz', users_factors=np.ones((4, 3)), items_factors=np.full((2, 3), 0.5))
    back.load_model_from_path(str(tmp_path))
    assert back.users_factors.dtype == torch.float32 and torch.equal(back.items_factors, torch.full((2, 3), 0.5))
    als = Sm.AlternatingLeastSquare(40, 3, 0.01, 1, device='cpu')
    als.users_factors, als.items_factors = torch.ones(4, 3), torch.ones(2, 3)
    als.save_model_to_path(str(tmp_path))
    with pytest.raises(ValueError, match='holds a AlternatingLeastSquare'):
        back.load_model_from_path(str(tmp_path))
    assert torch.equal(back.items_factors, torch.full((2, 3), 0.5))                 # a refused file leaves the model as it is


def test_ops_refuse_host_and_wrong_operands():
    Sm = S()
    feats = importlib.import_module(Sm.ops.__name__.rsplit('.', 1)[0] + '.features')
    csr = feats.DeviceCSR(sp.csr_matrix(np.eye(3)))
    for thunk in (lambda: Sm.ops.gram(torch.zeros(3, 4)), lambda: Sm.ops.sym_eig(torch.eye(4)),
                  lambda: Sm.ops.csr_times_dense(csr, torch.zeros(3, 4)), lambda: Sm.ops.rotate_cols(torch.zeros(3, 4), torch.eye(4)),
                  lambda: Sm.ops.col_residual(torch.zeros(3, 4), torch.zeros(3, 4), torch.ones(4), 2)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            thunk()


def test_header_declares_and_library_exports_the_entry_points():
    lib = importlib.import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')
    protos = lib.parse_header()
    assert protos['sbr_sym_eig_f32'][2] == ['A', 'n', 'lda', 'W', 'ldw', 'lam', 'info', 'workspace', 'workspace_bytes', 'stream']
    assert protos['sbr_sym_eig_f32_workspace'][0] is ctypes.c_long
    assert protos['sbr_gram_f32'][2] == ['Y', 'n_y', 'ldy', 'f', 'G', 'ldg', 'workspace', 'workspace_bytes', 'stream']
    assert protos['sbr_csr_times_dense_f32'][2] == ['indptr', 'indices', 'data', 'r0', 'r1', 'D', 'n_d', 'ldd', 'c', 'out', 'ldo', 'stream']
    assert protos['sbr_rotate_cols_f32'][2] == ['Y', 'n', 'ldy', 'b', 'W', 'ldw', 'lam', 's', 'out', 'ldo', 'stream']
    assert protos['sbr_col_residual_f32_workspace'][0] is ctypes.c_long
    text = open(os.path.join(ROOT, 'include', 'sibrar_hip.h')).read()
    for word in ('mf_algs.py:14-66', 'round robin', 'sign(tau) / (|tau| + sqrt(1 + tau^2))', 'the sweep cap is 30', 'largest magnitude'):
        assert word in text, word
    assert 'svd.hip' in open(os.path.join(os.path.dirname(lib.LIB_PATH), '..', 'csrc', 'Makefile')).read()
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name in ('sbr_sym_eig_f32', 'sbr_sym_eig_f32_workspace', 'sbr_gram_f32', 'sbr_csr_times_dense_f32', 'sbr_rotate_cols_f32', 'sbr_col_residual_f32',
                 'sbr_col_residual_f32_workspace'):
        assert hasattr(handle, name), name
    assert handle.sbr_abi_version() == 4
    # the argument checks come before anything touches the device: host arithmetic only
    handle.sbr_last_error.restype = ctypes.c_char_p
    L = lib.lib()
    assert L.sbr_col_residual_f32_workspace(257, 3) == 24 and L.sbr_col_residual_f32_workspace(0, 3) == 0
    for n, word in ((0, b'n=0'), (129, b'n=129')):
        assert L.sbr_sym_eig_f32(None, n, 200, None, 200, None, None, None, 0, None) != 0 and word in handle.sbr_last_error()
        assert L.sbr_sym_eig_f32_workspace(n) == 0
    assert L.sbr_sym_eig_f32(None, 4, 3, None, 4, None, None, None, 0, None) != 0 and b'leading dimension' in handle.sbr_last_error()
    assert L.sbr_sym_eig_f32_workspace(128) == 8 * 128 * 128 and L.sbr_sym_eig_f32_workspace(7) == 8 * 8 * 8
    assert L.sbr_gram_f32(None, 4, 8, 129, None, 129, None, 0, None) != 0 and b'sbr_gram_f32: f=129' in handle.sbr_last_error()
    assert L.sbr_als_gram_f32(None, 4, 8, 8, 0., None, 8, None, 0, None) != 0 and b'sbr_als_gram_f32: reg' in handle.sbr_last_error()
    times = L.sbr_csr_times_dense_f32
    for args, word in (((None, None, None, 0, 5, None, 4, 129, 129, None, 129, None), b'c=129'), ((None, None, None, 0, 5, None, 4, 8, 0, None, 8, None), b'c=0'),
                       ((None, None, None, 0, 5, None, 4, 7, 8, None, 8, None), b'leading dimension'),
                       ((None, None, None, 5, 4, None, 4, 8, 8, None, 8, None), b'row range'),
                       ((None, None, None, 0, 5, None, 4, 8, 8, None, 8, None), b'null operand')):
        assert times(*args) != 0 and word in handle.sbr_last_error() and b'sbr_csr_times_dense_f32' in handle.sbr_last_error(), word
    assert times(None, None, None, 3, 3, None, 4, 8, 8, None, 8, None) == 0                     # an empty range returns at once
