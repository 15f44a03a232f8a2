"""SLIM without a GPU: the Gram-form restatement of tests/slim_ref.py against the g26 fixture recorded from the reference (objective per
column, KKT residual of the optimum, the recorded pred_mtx), the restatement's two forms against each other, and the host side of
sibrar_amd.slim — registry, constructor, build_from_conf, the refusals, model.npz, the header and the library's exports."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import slim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS, CASES = R.load_g26()
IDS = [c['name'] for c in CASES]


def S():
    import sibrar_amd
    return sibrar_amd


def _penalties(case):
    return R.penalties(case['users'], case['alpha'], case['l1_ratio'])


def test_g26_covers_the_cases():
    assert [(c['alpha'], c['l1_ratio'], c['max_iter']) for c in CASES] == list(R.PARAMS) and IDS == [R.case_name(a, l) for a, l, _ in R.PARAMS]
    assert ARRAYS['inter'].shape == (50, 40) and set(np.unique(ARRAYS['inter'])) == {0., 1.}
    for c in CASES:
        assert c['model_name'] == 'SLIM' and c['users_left_out'] <= R.MAX_LEFT_OUT * c['users']
        for key in ('W_ref', 'W_opt'):
            w = ARRAYS[f'{c["name"]}/{key}']
            assert w.dtype == np.float64 and w.shape == (40, 40) and (w >= 0).all() and not np.diag(w).any()
        assert ARRAYS[c['name'] + '/pred_mtx'].shape == (50, 40)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_restatement_meets_the_reference(case):
    """per column the restatement's objective is within 1e-4 G_jj of the reference's; the recorded optimum satisfies KKT to 1e-8"""
    g = R.gram(ARRAYS['inter'])
    l1, l2 = _penalties(case)
    w, n_iter, _ = R.cd(g, l1, l2, case['max_iter'])
    w_ref, w_opt = ARRAYS[case['name'] + '/W_ref'], ARRAYS[case['name'] + '/W_opt']
    assert (n_iter > 0).all() and (w >= 0).all() and not np.diag(w).any()
    worst = max(abs(R.objective(g, j, w[:, j], l1, l2) - R.objective(g, j, w_ref[:, j], l1, l2)) / g[j, j] for j in range(40))
    below = max((R.objective(g, j, w_opt[:, j], l1, l2) - R.objective(g, j, w[:, j], l1, l2)) / g[j, j] for j in range(40))
    kkt = R.kkt_all(g, w_opt, l1, l2)
    print(f'{case["name"]}: objective distance from the reference {worst:.3e} G_jj, optimum above the restatement {below:.3e} G_jj, '
          f'KKT(W_opt) {kkt:.3e}, max |W - W_ref| {np.abs(w - w_ref).max():.3e}, sweeps <= {n_iter.max()}')
    assert worst <= R.OBJ_TOL and below <= 1e-12 and kkt <= 1e-8
    assert np.abs(w_opt - R.cd(g, l1, l2, 100000, 1e-12)[0]).max() == 0                  # W_opt is what the maker says it is
    left = int((~R.countable_users(ARRAYS[case['name'] + '/pred_mtx'], ARRAYS['inter'] @ w_opt, ARRAYS['inter'], R.FACTOR * case['e_ref'])).sum())
    assert left == case['users_left_out']


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_reference_weights_give_the_recorded_pred_mtx(case):
    pred = ARRAYS['inter'] @ ARRAYS[case['name'] + '/W_ref']
    assert np.abs(pred - ARRAYS[case['name'] + '/pred_mtx']).max() <= 1e-3             # two random runs of the reference


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_skipping_zero_steps_gives_the_plain_loop(dtype):
    """the search for the next coordinate with a non-zero step is the plain ascending loop, bit for bit, sweeps and steps included"""
    g = R.gram(ARRAYS['inter'])
    x = R.world(70, 45, 0.12, seed=5, empty_item=7, twin=(3, 30))
    for gm, n in ((g, 50), (R.gram(x), 70)):
        for alpha, l1_ratio in ((0.01, 0.5), (0.1, 0.9), (0.02, 0.), (0.02, 1.)):
            l1, l2 = R.penalties(n, alpha, l1_ratio)
            for tol, max_iter in ((R.TOL, 500), (0., 7)):
                a, b = R.cd(gm, l1, l2, max_iter, tol, dtype, skip=True), R.cd(gm, l1, l2, max_iter, tol, dtype, skip=False)
                assert a[0].dtype == dtype and all(np.array_equal(p, q) for p, q in zip(a, b)), (alpha, l1_ratio, tol)
    w = R.cd(R.gram(x), *R.penalties(70, 0.01, 0.5), 500)[0]
    assert not w[7].any() and not w[:, 7].any() and w[30, 3] > 0.3 and w[3, 30] > 0.3      # nobody's item; the twins name each other


def test_float32_restatement_is_fp32_close():
    g = R.gram(ARRAYS['inter'])
    for case in CASES:
        e, w64, w32 = R.e_ref(g, *_penalties(case), 50)
        assert 0 < e <= 1e-5 and np.abs(w64 - ARRAYS[case['name'] + '/W_opt']).max() <= 1e-3


def test_registry_constructor_and_conf():
    Sm = S()
    assert Sm.ALGORITHMS['slim'] is Sm.SLIM and issubclass(Sm.SLIM, Sm.SparseMatrixBasedRecommenderAlgorithm)
    m = Sm.SLIM(0.01, 0.5, 100, device='cpu')
    assert (m.name, m.alpha, m.l1_ratio, m.max_iter, m.tol, m.W, m.n_iter_, m.device) == ('SLIM', 0.01, 0.5, 100, 1e-4, None, None, torch.device('cpu'))
    assert (type(m).KEY, type(m).HYPER) == ('W', ('alpha', 'l1_ratio', 'max_iter', 'tol')) and type(m).STORES and type(m).BINARY_ONLY
    assert m.eval() is m and m.train() is m and m.to('cpu') is m
    assert Sm.SLIM(0.01, 0.5, 100).device == torch.device('cuda') and Sm.SLIM(0.01, 0.5, 100, tol=0.).tol == 0.
    assert m.penalties(50) == (50 * 0.01 * 0.5, 50 * 0.01 * 0.5) and Sm.SLIM(0.1, 0.9, 5).penalties(50) == R.penalties(50, 0.1, 0.9)
    m = Sm.SLIM.build_from_conf({'alg': 'slim', 'alpha': 0.001, 'l1_ratio': 0.1, 'max_iter': 500}, None)
    assert type(m) is Sm.SLIM and (m.alpha, m.l1_ratio, m.max_iter, m.tol) == (0.001, 0.1, 500, 1e-4)
    assert Sm.ALGORITHMS['slim'].build_from_conf({'alpha': 0, 'l1_ratio': 1, 'max_iter': 1}).max_iter == 1
    for missing in ('alpha', 'l1_ratio', 'max_iter'):
        conf = {'alpha': 0.01, 'l1_ratio': 0.5, 'max_iter': 10}
        del conf[missing]
        with pytest.raises(KeyError, match=missing):
            Sm.SLIM.build_from_conf(conf, None)


@pytest.mark.parametrize('args, kwargs, match', [((-0.01, 0.5, 10), {}, 'alpha'), ((float('nan'), 0.5, 10), {}, 'alpha'),
                                                 ((0.01, -0.1, 10), {}, 'l1_ratio'), ((0.01, 1.5, 10), {}, 'l1_ratio'),
                                                 ((0.01, 0.5, 0), {}, 'max_iter'), ((0.01, 0.5, 2.5), {}, 'max_iter'),
                                                 ((0.01, 0.5, 10), {'tol': -1e-4}, 'tol')])
def test_constructor_refusals(args, kwargs, match):
    with pytest.raises(ValueError, match=match):
        S().SLIM(*args, **kwargs)


def test_value_and_state_errors(tmp_path):
    Sm = S()
    with pytest.raises(ValueError, match='0/1'):
        Sm.SLIM(0.01, 0.5, 10, device='cpu').fit(sp.csr_matrix(np.array([[1., 2.], [0., 1.]])))
    dup = sp.coo_matrix((np.ones(3), ([0, 0, 1], [1, 1, 0])), shape=(2, 2))          # a duplicate entry sums to 2
    with pytest.raises(ValueError, match='Gram matrix'):
        Sm.SLIM(0.01, 0.5, 10, device='cpu').attach(dup)
    m = Sm.SLIM(0.01, 0.5, 10, device='cpu')
    with pytest.raises(RuntimeError, match='fit'):
        m.save_model_to_path(str(tmp_path))
    with pytest.raises(RuntimeError, match='fit'):
        m.predict(torch.tensor([0]), torch.tensor([[0]]))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.fit(sp.csr_matrix(np.eye(3)))                                            # a binary matrix gets as far as the first kernel
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Sm.ops.slim_weights(torch.eye(3), 1., 1., 10)


def test_model_npz(tmp_path):
    Sm = S()
    m = Sm.SLIM(0.01, 0.5, 100, device='cpu', tol=1e-5)
    m.W = torch.tensor([[0., 0.25], [0.5, 0.]])
    m.save_model_to_path(str(tmp_path))
    with np.load(tmp_path / 'model.npz', allow_pickle=False) as f:
        assert set(f.files) == {'W', 'alpha', 'l1_ratio', 'max_iter', 'tol', 'name'}
        assert (str(f['name']), float(f['alpha']), float(f['l1_ratio']), int(f['max_iter']), float(f['tol'])) == ('SLIM', 0.01, 0.5, 100, 1e-5)
    back = Sm.SLIM(0.01, 0.5, 100, device='cpu')
    back.load_model_from_path(str(tmp_path))
    assert torch.equal(back.W, m.W) and back.W.dtype == torch.float32
    with pytest.raises(RuntimeError, match='attach'):
        back.predict(torch.tensor([0]), torch.tensor([[0]]))                        # the file does not hold the interactions
    back.attach(sp.csr_matrix(np.ones((3, 2))))
    assert (back.n_users, back.n_items) == (3, 2)
    np.savez(tmp_path / 'model.npz', W=np.zeros((2, 3)), name=np.array('SLIM'))
    with pytest.raises(ValueError, match='not square'):
        back.load_model_from_path(str(tmp_path))
    np.savez(tmp_path / 'model.npz', W=np.zeros((2, 2)), name=np.array('EASE'))
    with pytest.raises(ValueError, match='holds a EASE'):
        back.load_model_from_path(str(tmp_path))


def test_a_reference_model_file_is_refused(tmp_path):
    np.savez(tmp_path / 'model.npz', pred_mtx=np.zeros((2, 2)))
    with pytest.raises(ValueError, match='pred_mtx'):
        S().SLIM(0.01, 0.5, 10).load_model_from_path(str(tmp_path))


def test_header_declares_and_library_exports_the_entry_point():
    lib = importlib.import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')
    protos = lib.parse_header()
    assert protos['sbr_slim_cd_f32'][2] == ['G', 'm', 'ldg', 'c0', 'c1', 'l1', 'l2', 'max_iter', 'tol', 'W', 'ldw', 'n_iter', 'stream']
    assert protos['sbr_slim_cd_f32'][1][5:9] == [ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_float]
    text = open(os.path.join(ROOT, 'include', 'sibrar_hip.h')).read()
    assert 'linear_algs.py:39-112' in text
    handle = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(handle, 'sbr_slim_cd_f32') and handle.sbr_abi_version() == 4
    # argument checks are host arithmetic: they answer without a device
    fn = handle.sbr_slim_cd_f32
    fn.restype, fn.argtypes = protos['sbr_slim_cd_f32'][:2]
    handle.sbr_last_error.restype = ctypes.c_char_p
    assert fn(None, 0, 0, 0, 0, 1., 1., 10, 1e-4, None, 0, None, None) == 0                       # m == 0: nothing to do
    assert fn(None, 5, 5, 2, 2, 1., 1., 10, 1e-4, None, 5, None, None) == 0                       # an empty range, before the operands
    for args, word in (((None, 5, 5, 0, 5, 1., 1., 10, 1e-4, None, 5, None, None), 'null operand'),
                       ((None, 5, 5, 3, 6, 1., 1., 10, 1e-4, None, 5, None, None), 'column range'),
                       ((None, 5, 4, 0, 5, 1., 1., 10, 1e-4, None, 5, None, None), 'leading dimension'),
                       ((None, 5, 5, 0, 5, -1., 1., 10, 1e-4, None, 5, None, None), 'penalties'),
                       ((None, 5, 5, 0, 5, 1., 1., 0, 1e-4, None, 5, None, None), 'max_iter'),
                       ((None, 5, 5, 0, 5, 1., 1., 10, -1., None, 5, None, None), 'tol'),
                       ((None, S().ops.SLIM_MAX_ITEMS + 1, 50000, 0, 0, 1., 1., 10, 1e-4, None, 50000, None, None), '160 KiB')):
        assert fn(*args) == 1 and word in handle.sbr_last_error().decode(), word
    assert S().ops.SLIM_MAX_ITEMS == (160 * 1024 - 512) // 4 >= 25000                             # the c5 catalogue fits
