"""P3alpha without a GPU: the float64 restatement of tests/p3alpha_ref.py against the g24 fixture recorded from the reference, the fp32
order oracle against that restatement within the derived bound, and the host side of sibrar_amd.p3alpha — registry, constructor,
build_from_conf, the ValueErrors, model.npz, the ops' refusals, the header and the library's exports."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import p3alpha_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS, CASES = R.load_g24()
IDS = [c['name'] for c in CASES]


def S():
    import sibrar_amd
    return sibrar_amd


def _feats():
    return importlib.import_module(S().ops.__name__.rsplit('.', 1)[0] + '.features')


def test_g24_covers_the_cases():
    assert IDS == [f'a{a}' for a in R.ALPHAS] + [f'empty/a{a}' for a in R.ALPHAS] and [c['alpha'] for c in CASES] == 2 * list(R.ALPHAS)
    for key in ('inter', 'inter_empty'):
        assert ARRAYS[key].shape == (50, 40) and set(np.unique(ARRAYS[key])) == {0., 1.}
    assert ARRAYS['inter'].sum(axis=1).min() > 0 and ARRAYS['inter'].sum(axis=0).min() > 0
    assert (ARRAYS['inter_empty'].sum(axis=1) == 0).sum() == 1 and (ARRAYS['inter_empty'].sum(axis=0) == 0).sum() == 1
    for c in CASES:
        assert c['model_name'] == 'P3alpha' and c['matrix'] == ('inter_empty' if c['name'].startswith('empty/') else 'inter')
        assert (c['empty_users'], c['empty_items']) == ((1, 1) if c['matrix'] == 'inter_empty' else (0, 0))
        assert c['users_left_out'] <= R.MAX_LEFT_OUT * c['users']
        pred = ARRAYS[c['name'] + '/pred_mtx']
        assert pred.dtype == np.float64 and pred.shape == (50, 40) and np.isfinite(pred).all() and pred.min() >= 0


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_restatement_meets_the_reference(case):
    inter, ref = ARRAYS[case['matrix']], ARRAYS[case['name'] + '/pred_mtx']
    w, pred = R.fit64(inter, case['alpha'])
    assert np.abs(pred - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.array_equal(pred == 0, ref == 0)                                     # empty users and items: zeros, not NaN
    if case['matrix'] == 'inter_empty':
        eu, ei = int(np.flatnonzero(inter.sum(axis=1) == 0)[0]), int(np.flatnonzero(inter.sum(axis=0) == 0)[0])
        assert not ref[eu].any() and not ref[:, ei].any() and not w[ei].any() and not w[:, ei].any()
    # the rows of W sum to one: the two steps item -> user -> item are a random walk
    held = inter.sum(axis=0) > 0
    assert np.allclose(w[held].sum(axis=1), 1., rtol=0, atol=1e-12)
    # the near-tie count the maker recorded is the one the rule gives on the fixture
    assert int((~R.countable_users(ref, inter, case['alpha'])).sum()) == case['users_left_out']


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_order_oracle_stays_within_the_bound(case):
    inter, ref = ARRAYS[case['matrix']], ARRAYS[case['name'] + '/pred_mtx']
    pre = R.pre_power32(inter, R.walk32(inter))
    assert pre.dtype == np.float32
    got = R.power64(pre, case['alpha'])                                            # an exact power: the bound's powf term is to spare
    err = np.abs(got - ref)
    worst = float((err / np.where(ref > 0, R.rel_bound(inter, case['alpha']) * ref, 1.)).max())
    print(f'P3alpha oracle {case["name"]}: worst error / bound {worst:.3f}')
    assert (err <= R.rel_bound(inter, case['alpha']) * ref).all() and np.array_equal(got == 0, ref == 0)


def test_order_oracle_on_the_worlds_of_the_gpu_tests():
    """the planted rows and columns are there, and the oracle meets float64 within the bound at alpha = 1 on each"""
    for name in ('50x40', '300x200', '97x130'):
        x = R.world(name, ARRAYS['inter'])
        n, m = x.shape
        du, di = np.diff(x.indptr), np.diff(sp.csr_matrix(x.T).tocsr().indptr)
        assert du[n - 2] == 0 and di[m - 3] == 0 and du[3] == m - 1 and di[5] == n - 1
        _, pred = R.fit64(x, 1.0)
        got = R.pre_power32(x, R.walk32(x)).astype(np.float64)
        assert (np.abs(got - pred) <= R.rel_bound(x, 1.0) * pred).all(), name
        assert not got[n - 2].any() and not got[:, m - 3].any()


def test_registry_constructor_and_conf():
    Sm = S()
    assert Sm.ALGORITHMS['p3alpha'] is Sm.P3alpha and issubclass(Sm.P3alpha, Sm.SparseMatrixBasedRecommenderAlgorithm)
    mod = importlib.import_module(Sm.P3alpha.__module__)
    assert mod.SparseMatrixBasedRecommenderAlgorithm is importlib.import_module(Sm.KNNAlgorithm.__module__).SparseMatrixBasedRecommenderAlgorithm
    m = Sm.P3alpha(device='cpu')
    assert (m.name, m.alpha, m.W, m.device) == ('P3alpha', 1.9, None, torch.device('cpu'))
    assert m.eval() is m and m.train() is m and m.to('cpu') is m
    assert Sm.P3alpha(0.5).device == torch.device('cuda')
    m = Sm.P3alpha.build_from_conf({'alg': 'p3alpha', 'alpha': 0.7}, None)
    assert type(m) is Sm.P3alpha and m.alpha == 0.7
    assert Sm.ALGORITHMS['p3alpha'].build_from_conf({'alpha': 1}).alpha == 1
    with pytest.raises(KeyError):
        Sm.P3alpha.build_from_conf({'alg': 'p3alpha'}, None)
    for text in ('0/1', 'alpha == 0', 'fp32'):
        assert text in mod.__doc__                                                 # the deliberate differences are stated


def test_alpha_below_zero_and_zero_are_refused():
    with pytest.raises(ValueError, match='greater or equal than 0'):
        S().P3alpha(-0.1)
    with pytest.raises(ValueError, match='scipy refuses a zero power'):
        S().P3alpha(0)
    with pytest.raises(ValueError, match='reference'):
        S().P3alpha.build_from_conf({'alpha': 0.0})


def test_value_and_state_errors(tmp_path):
    Sm = S()
    with pytest.raises(ValueError, match='0/1'):
        Sm.P3alpha(1, device='cpu').fit(sp.csr_matrix(np.array([[1., 2.], [0., 1.]])))
    dup = sp.coo_matrix((np.ones(3), ([0, 0, 1], [1, 1, 0])), shape=(2, 2))          # a duplicate entry sums to 2
    with pytest.raises(ValueError, match='entry counts'):
        Sm.P3alpha(1, device='cpu').attach(dup)
    m = Sm.P3alpha(1, device='cpu')
    with pytest.raises(RuntimeError, match='fit'):
        m.save_model_to_path(str(tmp_path))
    with pytest.raises(RuntimeError, match='fit'):
        m.predict(torch.tensor([0]), torch.tensor([[0]]))
    with pytest.raises(RuntimeError, match='fit'):
        m.combine_user_item_representations(m.get_user_representations(torch.tensor([0])), m.get_item_representations(torch.tensor([0])))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.fit(sp.csr_matrix(np.eye(3)))                                            # a binary matrix gets as far as the first kernel


def test_model_npz(tmp_path):
    Sm = S()
    m = Sm.P3alpha(0.5, device='cpu')
    m.W = torch.tensor([[0.75, 0.25], [0.5, 0.5]])
    m.save_model_to_path(str(tmp_path))
    with np.load(tmp_path / 'model.npz', allow_pickle=False) as f:
        assert set(f.files) == {'W', 'alpha', 'name'} and (str(f['name']), float(f['alpha'])) == ('P3alpha', 0.5)
    back = Sm.P3alpha(0.5, device='cpu')
    back.load_model_from_path(str(tmp_path))
    assert torch.equal(back.W, m.W) and back.W.dtype == torch.float32
    with pytest.raises(RuntimeError, match='attach'):
        back.predict(torch.tensor([0]), torch.tensor([[0]]))                        # the file does not hold the interactions
    back.attach(sp.csr_matrix(np.ones((3, 2))))
    assert (back.n_users, back.n_items) == (3, 2)
    np.savez(tmp_path / 'model.npz', W=np.zeros((2, 3)), alpha=np.array(1.), name=np.array('P3alpha'))
    with pytest.raises(ValueError, match='not square'):
        back.load_model_from_path(str(tmp_path))
    np.savez(tmp_path / 'model.npz', W=np.zeros((2, 2)), alpha=np.array(1.), name=np.array('EASE'))
    with pytest.raises(ValueError, match='holds a EASE'):
        back.load_model_from_path(str(tmp_path))


def test_a_reference_model_file_is_refused(tmp_path):
    np.savez(tmp_path / 'model.npz', pred_mtx=np.zeros((2, 2)))
    with pytest.raises(ValueError, match='pred_mtx'):
        S().P3alpha(1).load_model_from_path(str(tmp_path))
    np.savez(tmp_path / 'model.npz', pred_mtx=sp.csr_matrix(np.eye(2)))              # what the reference writes: a pickled object array
    with pytest.raises(ValueError, match='pred_mtx'):
        S().P3alpha(1).load_model_from_path(str(tmp_path))


def test_ops_refuse_host_and_wrong_operands():
    Sm = S()
    csr = _feats().DeviceCSR(sp.csr_matrix(np.eye(3)))
    w = torch.zeros(3, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Sm.ops.p3_walk_dense(csr)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Sm.ops.p3_score_rows(csr, torch.tensor([0]), w, 1.)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Sm.ops.p3_score_rows(csr, None, w, 1.)
    valued = _feats().DeviceCSR(sp.csr_matrix(np.eye(3) * 2))
    with pytest.raises(ValueError, match='0/1'):
        Sm.ops.p3_walk_dense(valued)
    with pytest.raises(ValueError, match='0/1'):
        Sm.ops.p3_score_rows(valued, None, w, 1.)
    for bad in (w.double(), torch.zeros(3, 4), torch.zeros(4, 4), torch.zeros(9), torch.zeros(3, 6)[:, ::2]):
        with pytest.raises(ValueError, match=r'contiguous float32 \[3, 3\]'):
            Sm.ops.p3_score_rows(csr, None, bad, 1.)
    for alpha in (0, -1.5, float('nan')):
        with pytest.raises(ValueError, match='must be positive'):
            Sm.ops.p3_score_rows(csr, None, w, alpha)


def test_header_declares_and_library_exports_the_entry_points():
    lib = importlib.import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')
    protos = lib.parse_header()
    assert protos['sbr_p3_walk_dense'][2] == ['indptr', 'indices', 't_indptr', 't_indices', 'n', 'm', 'r0', 'r1', 'tile_cols', 'W', 'ld', 'stream']
    assert protos['sbr_p3_score_rows'][2] == ['indptr', 'indices', 'rows', 'B', 'W', 'ldw', 'm', 'alpha', 'out', 'ldo', 'stream']
    assert protos['sbr_p3_score_rows'][1][3] is ctypes.c_long and protos['sbr_p3_score_rows'][1][7] is ctypes.c_float
    text = open(os.path.join(ROOT, 'include', 'sibrar_hip.h')).read()
    assert 'graph_algs.py:35-59' in text and 'graph_algs.py:59-68' in text and 'in ascending v' in text
    assert 'p3alpha.hip' in open(os.path.join(os.path.dirname(lib.LIB_PATH), '..', 'csrc', 'Makefile')).read()
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name in ('sbr_p3_walk_dense', 'sbr_p3_score_rows'):
        assert hasattr(handle, name), name
    assert handle.sbr_abi_version() == 4
    # the argument checks come before anything touches the device: host arithmetic only
    handle.sbr_last_error.restype = ctypes.c_char_p
    walk = getattr(lib.lib(), 'sbr_p3_walk_dense')
    assert walk(None, None, None, None, 5, 4, 0, 5, 0, None, 4, None) != 0 and b'row range' in handle.sbr_last_error()
    assert walk(None, None, None, None, 5, 50000, 0, 50000, 50000, None, 50000, None) != 0 and b'160 KiB' in handle.sbr_last_error()
    assert walk(None, None, None, None, 5, 4, 2, 2, 0, None, 4, None) == 0           # an empty range returns at once
    score = getattr(lib.lib(), 'sbr_p3_score_rows')
    assert score(None, None, None, 3, None, 4, 4, 0., None, 4, None) != 0 and b'alpha' in handle.sbr_last_error()
    assert score(None, None, None, 3, None, 3, 4, 1., None, 4, None) != 0 and b'bad shape' in handle.sbr_last_error()
    assert score(None, None, None, 0, None, 4, 4, 1., None, 4, None) == 0
