"""EASE without a GPU: the float64 restatement of tests/ease_ref.py against the g23 fixture recorded from the reference, the blocked sweep of
ease_ref.py against np.linalg.inv, and the host side of sibrar_amd.ease — registry, constructor, build_from_conf, the int(lam) rule, the
ValueErrors, model.npz, the header and the library's exports."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import ease_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS, CASES = R.load_g23()


def S():
    import sibrar_amd
    return sibrar_amd


def test_g23_covers_the_cases():
    assert [c['name'] for c in CASES] == ['lam1', 'lam10', 'lam500'] and [c['lam'] for c in CASES] == list(R.LAMS)
    assert ARRAYS['inter'].shape == (50, 40) and set(np.unique(ARRAYS['inter'])) == {0., 1.}
    for c in CASES:
        assert c['diag'] == int(c['lam']) and c['model_name'] == 'EASE'
        assert c['users_left_out'] <= R.MAX_LEFT_OUT * c['users']
        assert ARRAYS[c['name'] + '/B'].dtype == np.float64 and ARRAYS[c['name'] + '/pred_mtx'].shape == (50, 40)


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_restatement_meets_the_reference(case):
    b, pred = R.fit64(ARRAYS['inter'], case['lam'])
    for got, key in ((b, 'B'), (pred, 'pred_mtx')):
        ref = ARRAYS[f'{case["name"]}/{key}']
        assert np.abs(got - ref).max() <= 1e-10 * np.abs(ref).max(), key
    assert np.all(np.diag(b) == 0) and not np.allclose(b, b.T)                    # column scaling: B is not symmetric
    # the near-tie count the maker recorded is the one the rule gives on the fixture
    assert int((~R.countable_users(ARRAYS[case['name'] + '/pred_mtx'], ARRAYS['inter'], case['e_ref_weights'])).sum()) == case['users_left_out']


def test_truncation_of_lam_shows_in_the_fixture():
    b500, _ = R.fit64(ARRAYS['inter'], 500)
    b501, _ = R.fit64(ARRAYS['inter'], 501)
    ref = ARRAYS['lam500/B']
    assert np.abs(b500 - ref).max() <= 1e-10 * np.abs(ref).max() < np.abs(b501 - ref).max()


@pytest.mark.parametrize('n', [1, 40, 64, 65, 130, 200])
def test_sweep_inverse_float64(n):
    for lam in (1, 500):
        a = R.random_spd(n, lam, seed=n + lam)
        inv = np.linalg.inv(a)
        got, info = R.sweep_inverse(a, return_info=True)
        assert info == 0 and np.abs(got - inv).max() <= 1e-9 * np.abs(inv).max(), (n, lam)
        assert R.e_ref(a) <= 1e-4 * np.abs(inv).max()                              # and the fp32 yardstick is an fp32-sized error


def test_sweep_inverse_names_the_first_bad_pivot():
    d = np.ones(130)
    d[69] = 0
    assert R.sweep_inverse(np.diag(d), dtype=np.float32, return_info=True)[1] == 70
    assert R.sweep_inverse(-np.eye(3), return_info=True)[1] == 1


def test_registry_constructor_and_conf():
    Sm = S()
    assert Sm.ALGORITHMS['ease'] is Sm.EASE and issubclass(Sm.EASE, Sm.SparseMatrixBasedRecommenderAlgorithm)
    ease = importlib.import_module(Sm.EASE.__module__)
    assert ease.SparseMatrixBasedRecommenderAlgorithm is importlib.import_module(Sm.KNNAlgorithm.__module__).SparseMatrixBasedRecommenderAlgorithm
    m = Sm.EASE(500.7, device='cpu')
    assert (m.name, m.lam, m.B, m.device) == ('EASE', 500.7, None, torch.device('cpu'))
    assert m.eval() is m and m.train() is m and m.to('cpu') is m
    assert Sm.EASE(3).device == torch.device('cuda')
    m = Sm.EASE.build_from_conf({'alg': 'ease', 'lam': 20}, None)
    assert type(m) is Sm.EASE and m.lam == 20
    m = Sm.ALGORITHMS['ease'].build_from_conf({'lam': 1.9})
    assert m.lam == 1.9
    with pytest.raises(KeyError):
        Sm.EASE.build_from_conf({'alg': 'ease'}, None)


@pytest.mark.parametrize('lam', [0, 0.99, -3, -0.5])
def test_lam_below_one_is_refused(lam):
    with pytest.raises(ValueError, match=r'int\(lam\)'):
        S().EASE(lam)


def test_value_and_state_errors(tmp_path):
    Sm = S()
    with pytest.raises(ValueError, match='0/1'):
        Sm.EASE(1, device='cpu').fit(sp.csr_matrix(np.array([[1., 2.], [0., 1.]])))
    dup = sp.coo_matrix((np.ones(3), ([0, 0, 1], [1, 1, 0])), shape=(2, 2))          # a duplicate entry sums to 2
    with pytest.raises(ValueError, match='integer counts'):
        Sm.EASE(1, device='cpu').attach(dup)
    m = Sm.EASE(1, device='cpu')
    with pytest.raises(RuntimeError, match='fit'):
        m.save_model_to_path(str(tmp_path))
    with pytest.raises(RuntimeError, match='fit'):
        m.predict(torch.tensor([0]), torch.tensor([[0]]))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.fit(sp.csr_matrix(np.eye(3)))                                            # a binary matrix gets as far as the first kernel


def test_model_npz(tmp_path):
    Sm = S()
    m = Sm.EASE(7.5, device='cpu')
    m.B = torch.tensor([[0., 0.25], [-0.5, 0.]])
    m.save_model_to_path(str(tmp_path))
    with np.load(tmp_path / 'model.npz', allow_pickle=False) as f:
        assert set(f.files) == {'B', 'lam', 'name'} and (str(f['name']), float(f['lam'])) == ('EASE', 7.5)
    back = Sm.EASE(7.5, device='cpu')
    back.load_model_from_path(str(tmp_path))
    assert torch.equal(back.B, m.B) and back.B.dtype == torch.float32
    with pytest.raises(RuntimeError, match='attach'):
        back.predict(torch.tensor([0]), torch.tensor([[0]]))                        # the file does not hold the interactions
    back.attach(sp.csr_matrix(np.ones((3, 2))))
    assert (back.n_users, back.n_items) == (3, 2)
    np.savez(tmp_path / 'model.npz', B=np.zeros((2, 3)), lam=np.array(1), name=np.array('EASE'))
    with pytest.raises(ValueError, match='not square'):
        back.load_model_from_path(str(tmp_path))


def test_a_reference_model_file_is_refused(tmp_path):
    np.savez(tmp_path / 'model.npz', pred_mtx=np.zeros((2, 2)))
    with pytest.raises(ValueError, match='pred_mtx'):
        S().EASE(1).load_model_from_path(str(tmp_path))


def test_ops_refuse_host_and_wrong_operands():
    Sm = S()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Sm.ops.spd_inverse_(torch.eye(3))
    feats = importlib.import_module(Sm.ops.__name__.rsplit('.', 1)[0] + '.features')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Sm.ops.gram_dense(feats.DeviceCSR(sp.csr_matrix(np.eye(3))))


def test_header_declares_and_library_exports_the_entry_points():
    lib = importlib.import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')
    protos = lib.parse_header()
    assert len(protos['sbr_gram_dense'][1]) == 13 and protos['sbr_gram_dense'][2][8:12] == ['diag_add', 'tile_cols', 'G', 'ld']
    assert protos['sbr_spd_inverse_f32'][2] == ['A', 'n', 'ld', 'workspace', 'workspace_bytes', 'info', 'stream']
    assert protos['sbr_spd_inverse_f32_workspace'][0] is ctypes.c_long and protos['sbr_spd_inverse_f32_workspace'][2] == ['n']
    assert protos['sbr_ease_weights_f32'][2] == ['P', 'n', 'ld', 'diag', 'stream']
    text = open(os.path.join(ROOT, 'include', 'sibrar_hip.h')).read()
    assert 'linear_algs.py:150-153' in text and 'linear_algs.py:155' in text and 'linear_algs.py:157-158' in text
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name in ('sbr_gram_dense', 'sbr_spd_inverse_f32', 'sbr_spd_inverse_f32_workspace', 'sbr_ease_weights_f32'):
        assert hasattr(handle, name), name
    ws = handle.sbr_spd_inverse_f32_workspace
    ws.restype, ws.argtypes = ctypes.c_long, [ctypes.c_int]
    # D^-1 [64, 64] and two panels [64, n rounded up to 128]; host arithmetic only
    assert [ws(n) for n in (0, 1, 128, 129)] == [0, 4 * (4096 + 2 * 64 * 128), 4 * (4096 + 2 * 64 * 128), 4 * (4096 + 2 * 64 * 256)]
    assert handle.sbr_abi_version() == 4
