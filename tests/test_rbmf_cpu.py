"""RBMF without a GPU: the numpy restatement of tests/rbmf_ref.py checks itself (its certificate max |U inv(U[idx])| <= tol holds on
every input the GPU tests use, in float64 and in float32), and the host side of sibrar_amd.rbmf — registry, constructor,
build_from_conf, the refusals, model.npz in both spellings, the header and the library's exports and argument checks."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import rbmf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RS = (1, 2, 63, 64, 65, 100, 128)
SLAB = 160                                                                         # the slab of the kernel-level GPU tests


def S():
    import sibrar_amd
    return sibrar_amd


def sizes(r):
    return sorted({n for n in (r, r + 1, SLAB - 1, SLAB + 1, 3 * SLAB + 7) if n >= r})


@pytest.mark.parametrize('r', RS)
def test_the_restatement_meets_its_certificate(r):
    for n in sizes(r):
        u, idx, L, ltop, utop, ratio = R.lu_input(n, r)
        assert sorted(set(idx)) == sorted(idx) and ratio <= 1 - 1e-3
        assert np.abs(L @ utop - u).max() <= 1e-12 and np.abs(np.tril(L[idx]) - ltop).max() == 0      # float64: u = L Utop, row by row
        u2, i64, s64, i32, s32, ratio2 = R.poor_start_input(n, r)
        c64, c32 = R.certificate(u2, i64), R.certificate(u2, i32)
        print(f'r={r} n={n}: LU ratio {ratio:.5f}; poor start: {s64} swaps (float32 {s32}), ratio {ratio2:.5f}, certificate {c64:.6f} (float32 {c32:.6f})')
        assert c64 <= R.TOL * (1 + 1e-12) and c32 <= R.TOL + R.slack(u2, i32, r)
        assert set(i64) == set(i32) and s64 == s32
        if n > r:
            assert s64 >= 1 and R.certificate(u2, np.arange(r)) > R.TOL               # the start was poor
        i0, s0, _ = R.maxvol(u2, max_iters=0, start=np.arange(r))
        assert s0 == 0 and np.array_equal(i0, np.arange(r))


@pytest.mark.parametrize('name', list(R.WORLDS))
def test_the_worlds_need_swaps_and_float32_agrees(name):
    """recorded here with numpy's float32 SVD as U: 5, 12 and 20 swaps, worst decision ratios 0.9975, 0.9979 and 0.99986"""
    nu, ni, g, p_in, p_out, seed, r = R.WORLDS[name]
    x = R.planted(nu, ni, g, p_in, p_out, seed)
    u = np.ascontiguousarray(np.linalg.svd(np.asarray(x.todense(), dtype=np.float32), full_matrices=False)[0][:, :r])
    i64, s64, ratio = R.maxvol(u)
    i32, s32, _ = R.maxvol(u, dtype=np.float32)
    print(f'{name}: {s64} swaps (float32 {s32}), worst ratio {ratio:.5f}, certificate {R.certificate(u, i64):.6f}')
    assert s64 >= 3 and s64 < R.MAX_ITERS and R.certificate(u, i64) <= R.TOL * (1 + 1e-12)
    assert ratio > R.RATIO_MAX or (set(i64) == set(i32) and s64 == s32)
    x64, c = R.ridge(x, i64, 1e-2)
    k = c.T @ c + 1e-2 * np.eye(r)
    assert np.abs(x64 @ k - np.asarray(x @ c)).max() <= 1e-9 * np.abs(k).max()       # X (C C^T + lam I) = matrix C^T


def test_registry_constructor_and_conf():
    Sm = S()
    cls = Sm.RBMF
    assert Sm.ALGORITHMS['rbmf'] is cls and issubclass(cls, Sm.FactorModel) and issubclass(cls, Sm.SparseMatrixBasedRecommenderAlgorithm)
    m = cls.build_from_conf({'alg': 'rbmf', 'n_representatives': 64, 'lam': 0.5}, None)
    assert type(m) is cls and (m.name, m.n_representatives, m.lam, m.tol, m.max_iters) == ('RBMF', 64, 0.5, 1.05, 100)
    assert (m.oversample, m.n_iterations, m.svd_tol, m.random_state) == (28, 100, 1e-5, 0) and m.device == torch.device('cuda')
    assert m.X is None and m.C is None and m.users_factors is None and m.representatives is None and m.n_swaps is None
    assert cls(8).lam == 1e-2 and cls(120).oversample == 8 and m.eval() is m and m.train() is m
    for missing in ('n_representatives', 'lam'):
        conf = {'n_representatives': 4, 'lam': 0.1}
        del conf[missing]
        with pytest.raises(KeyError):
            cls.build_from_conf(conf, None)
    m = cls(5, 0.3, device='cpu', random_state=7, tol=1.2, max_iters=9, oversample=3, n_iterations=11, svd_tol=1e-4)
    assert (m.device, m.random_state, m.tol, m.max_iters, m.oversample, m.n_iterations, m.svd_tol) == (torch.device('cpu'), 7, 1.2, 9, 3, 11, 1e-4)
    assert np.array_equal(m.initial_block(11, 8), np.random.RandomState(7).standard_normal(size=(11, 8)).astype(np.float32))
    m.X, m.C = torch.ones(2, 5), torch.zeros(3, 5)                                    # the reference's names are the factors
    assert m.users_factors is m.X and m.items_factors is m.C and tuple(m.items_factors.shape) == (3, 5)
    mod = importlib.import_module(cls.__module__)
    for text in ('maxvolpy', 'Goreinov', 'unchecked', 'lam = 0', 'Cholesky', 'n_representatives <= 128'):
        assert text in mod.__doc__
    assert Sm.ops.MAXVOL_MAX_R == 128 and Sm.ops.MAXVOL_GROUP == 16


def test_refusals(tmp_path):
    cls = S().RBMF
    for r in (129, 0, -3, 2.5):
        with pytest.raises(ValueError, match='n_representatives'):
            cls(r)
    for lam in (0, -1e-2, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='lam'):
            cls(4, lam)
    for kw, word in (({'tol': 0.99}, 'tol'), ({'tol': float('nan')}, 'tol'), ({'max_iters': -1}, 'max_iters'), ({'max_iters': 1.5}, 'max_iters'),
                     ({'oversample': -1}, 'oversample'), ({'n_iterations': 0}, 'n_iterations'), ({'svd_tol': float('nan')}, 'svd_tol')):
        with pytest.raises(ValueError, match=word):
            cls(4, **kw)
    m = cls(4, device='cpu')
    with pytest.raises(ValueError, match=r'n_representatives \(4\) exceeds min\(n_users, n_items\) = 3'):
        m.fit(sp.csr_matrix(np.eye(3)))
    d = np.eye(5)
    d[2, 3] = np.nan
    with pytest.raises(ValueError, match='non-finite'):
        m.fit(sp.csr_matrix(d))
    with pytest.raises(RuntimeError, match='fit'):
        m.save_model_to_path(str(tmp_path))
    with pytest.raises(RuntimeError, match='fit'):
        m.predict(torch.tensor([0]), torch.tensor([[0]]))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.fit(sp.csr_matrix(-np.eye(6) * 2.5))                                     # any finite values get as far as the first kernel


def test_model_npz(tmp_path):
    Sm = S()
    m = Sm.RBMF(3, device='cpu')
    m.X, m.C = torch.arange(12.).view(4, 3), torch.arange(6.).view(2, 3) / 4
    m.save_model_to_path(str(tmp_path))
    with np.load(tmp_path / 'model.npz', allow_pickle=False) as f:
        assert set(f.files) == {'X', 'C', 'name'} and str(f['name']) == 'RBMF' and f['C'].shape == (2, 3)
    back = Sm.RBMF(3, device='cpu')
    back.load_model_from_path(str(tmp_path))                                       # no device is needed, and no attach
    assert torch.equal(back.X, m.X) and torch.equal(back.C, m.C)
    u, i = torch.tensor([3, 0]), torch.tensor([1, 0])
    assert torch.equal(back.get_user_representations(u), m.X[u]) and torch.equal(back.get_item_representations(i), m.C[i])
    # a file written the reference's way (algorithms/mf_algs.py:197-200): float64 X and C, no name
    np.savez(tmp_path / 'model.npz', X=np.ones((4, 3)), C=np.full((2, 3), 0.5))
    back.load_model_from_path(str(tmp_path))
    assert back.X.dtype == torch.float32 and torch.equal(back.C, torch.full((2, 3), 0.5))
    # the other factor models' files are not RBMF's, and theirs keep their fields
    svd = Sm.SVDAlgorithm(3, device='cpu')
    svd.users_factors, svd.items_factors = torch.ones(4, 3), torch.ones(2, 3)
    svd.save_model_to_path(str(tmp_path))
    with np.load(tmp_path / 'model.npz', allow_pickle=False) as f:
        assert set(f.files) == {'users_factors', 'items_factors', 'name'}
    with pytest.raises(ValueError, match='not a model of this package'):
        back.load_model_from_path(str(tmp_path))
    assert torch.equal(back.C, torch.full((2, 3), 0.5))                             # a refused file leaves the model as it is
    m.save_model_to_path(str(tmp_path))
    with pytest.raises(ValueError, match='not a model of this package'):
        svd.load_model_from_path(str(tmp_path))


def test_ops_refuse_host_and_wrong_operands():
    ops = S().ops
    for thunk in (lambda: ops.maxvol(torch.zeros(5, 3)), lambda: ops.maxvol_lu(torch.zeros(5, 3)), lambda: ops.cholesky(torch.eye(4)),
                  lambda: ops.tri_solve_rows(torch.zeros(5, 4), torch.eye(4))):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            thunk()


def test_header_declares_and_library_exports_the_entry_points():
    lib = importlib.import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')
    protos = lib.parse_header()
    assert protos['sbr_maxvol_lu_step_f32'][2] == ['A', 'n', 'lda', 'r', 'k', 'idx', 'Ltop', 'ldl', 'Utop', 'ldu', 'info', 'workspace',
                                                   'workspace_bytes', 'slab_rows', 'stream']
    assert protos['sbr_tri_solve_rows_f32'][2] == ['in', 'ldi', 'n', 'r', 'T', 'ldt', 'upper', 'unit', 'out', 'ldo', 'stream']
    assert protos['sbr_maxvol_swap_step_f32'][2] == ['B', 'n', 'ldb', 'r', 'tol', 's', 'idx', 'n_swaps', 'workspace', 'workspace_bytes',
                                                     'slab_rows', 'stream']
    assert protos['sbr_chol_f32'][2] == ['K', 'n', 'ldk', 'R', 'ldr', 'info', 'stream']
    assert protos['sbr_maxvol_f32_workspace'][0] is ctypes.c_long
    text = open(os.path.join(ROOT, 'include', 'sibrar_hip.h')).read()
    assert text.count('mf_algs.py:168-186') >= 5
    for word in ('Goreinov', 'r * 2^-24', 'the lowest row, then the lowest column', 'no cooperative launch', 'chol_lds.h'):
        assert word in text, word
    assert 'rbmf.hip' in open(os.path.join(os.path.dirname(lib.LIB_PATH), '..', 'csrc', 'Makefile')).read()
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name in ('sbr_maxvol_lu_step_f32', 'sbr_maxvol_swap_step_f32', 'sbr_tri_solve_rows_f32', 'sbr_chol_f32', 'sbr_maxvol_f32_workspace'):
        assert hasattr(handle, name), name
    assert handle.sbr_abi_version() == 4
    # the argument checks come before anything touches the device: host arithmetic only
    handle.sbr_last_error.restype = ctypes.c_char_p
    L = lib.lib()
    assert L.sbr_maxvol_f32_workspace(1000, 0) == 4 * (6 * 4 + 1000 + 4) and L.sbr_maxvol_f32_workspace(1000, 160) == 4 * (6 * 7 + 1000 + 4)
    assert L.sbr_maxvol_f32_workspace(0, 0) == 0 and L.sbr_maxvol_f32_workspace(10, 1025) == 0 and L.sbr_maxvol_f32_workspace(10, -1) == 0
    lu, swap, tri, chol = L.sbr_maxvol_lu_step_f32, L.sbr_maxvol_swap_step_f32, L.sbr_tri_solve_rows_f32, L.sbr_chol_f32
    buf = ctypes.create_string_buffer(1 << 16)                                     # a host buffer: big enough, and never dereferenced
    ws = ctypes.addressof(buf)
    for args, word in (((None, 10, 4, 0, 0, None, None, 4, None, 4, None, ws, 1 << 16, 0, None), b'r=0'),
                       ((None, 10, 200, 129, 0, None, None, 200, None, 200, None, ws, 1 << 16, 0, None), b'r=129'),
                       ((None, 3, 4, 4, 0, None, None, 4, None, 4, None, ws, 1 << 16, 0, None), b'n=3'),
                       ((None, 10, 3, 4, 0, None, None, 4, None, 4, None, ws, 1 << 16, 0, None), b'leading dimension'),
                       ((None, 10, 4, 4, 0, None, None, 4, None, 4, None, ws, 1 << 16, 2000, None), b'slab_rows=2000'),
                       ((None, 10, 4, 4, 0, None, None, 4, None, 4, None, ws, 8, 0, None), b'workspace of 8 bytes'),
                       ((None, 10, 4, 4, 0, None, None, 4, None, 4, None, None, 1 << 16, 0, None), b'workspace'),
                       ((None, 10, 4, 4, 4, None, None, 4, None, 4, None, ws, 1 << 16, 0, None), b'step k=4'),
                       ((None, 10, 4, 4, 0, None, None, 3, None, 4, None, ws, 1 << 16, 0, None), b'leading dimension'),
                       ((None, 10, 4, 4, 0, None, None, 4, None, 4, None, ws, 1 << 16, 0, None), b'null operand')):
        assert lu(*args) != 0 and word in handle.sbr_last_error() and b'sbr_maxvol_lu_step_f32' in handle.sbr_last_error(), word
    for args, word in (((None, 10, 4, 4, 1.05, 0, None, None, ws, 1 << 16, 0, None), b'null operand'),
                       ((None, 10, 4, 4, 0.5, 0, None, None, ws, 1 << 16, 0, None), b'tol=0.5'),
                       ((None, 10, 4, 4, float('nan'), 0, None, None, ws, 1 << 16, 0, None), b'tol='),
                       ((None, 10, 4, 4, 1.05, -1, None, None, ws, 1 << 16, 0, None), b'step s=-1'),
                       ((None, 10, 4, 200, 1.05, 0, None, None, ws, 1 << 16, 0, None), b'r=200')):
        assert swap(*args) != 0 and word in handle.sbr_last_error() and b'sbr_maxvol_swap_step_f32' in handle.sbr_last_error(), word
    for args, word in (((None, 4, 5, 4, None, 4, 0, 0, None, 4, None), b'null operand'), ((None, 4, 5, 129, None, 200, 0, 0, None, 200, None), b'r=129'),
                       ((None, 3, 5, 4, None, 4, 0, 0, None, 4, None), b'leading dimension'), ((None, 4, 5, 4, None, 4, 2, 0, None, 4, None), b'flags'),
                       ((None, 4, -1, 4, None, 4, 0, 0, None, 4, None), b'n=-1')):
        assert tri(*args) != 0 and word in handle.sbr_last_error() and b'sbr_tri_solve_rows_f32' in handle.sbr_last_error(), word
    assert tri(None, 4, 0, 4, None, 4, 0, 0, None, 4, None) == 0                      # no rows: returns at once
    for args, word in (((None, 0, 4, None, 4, None, None), b'n=0'), ((None, 129, 200, None, 200, None, None), b'n=129'),
                       ((None, 4, 3, None, 4, None, None), b'leading dimension'), ((None, 4, 4, None, 4, None, None), b'null operand')):
        assert chol(*args) != 0 and word in handle.sbr_last_error() and b'sbr_chol_f32' in handle.sbr_last_error(), word
