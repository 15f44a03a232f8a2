"""csrc/ease.hip on the GPU: sbr_gram_dense exactly against scipy, sbr_spd_inverse_f32 against float64 np.linalg.inv with the error of the
fp32 restatement of the same sweep (tests/ease_ref.py) as the yardstick — kernel error <= 8 e_ref: another fixed summation order and fma
chains carry errors of the same size, not the same value — and EASE against the g23 fixture recorded from the reference, through
evaluate_recommender_algorithm, in deterministic mode and through model.npz. Every ratio is printed before it is asserted."""
import functools
import importlib
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import ease_ref as R
import evalk_ref as E
from hip_testutil import DEV, S, _Buf, _i32, _i64, _L, _p, call

pytestmark = pytest.mark.gpu

ARRAYS, CASES = R.load_g23()
SENTINEL = 7.25


def _feats():
    return importlib.import_module(S().ops.__name__.rsplit('.', 1)[0] + '.features')


# ---- sbr_gram_dense ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gram_matrix(name):
    if name == '50x40':
        return sp.csr_matrix(ARRAYS['inter'])
    n, m = (300, 200) if name == '300x200' else (97, 130)
    d = np.random.default_rng(n + m).random((n, m)) < 0.1
    if name == '97x130':
        d[:, 17] = False                    # an empty column: a row and a column of zeros in G
        d[40] = False                       # an empty row
    x = sp.csr_matrix(d.astype(np.float64))
    x.sort_indices()
    return x


def gram_ref(x, diag_add):
    return np.asarray((x.T @ x).todense()) + diag_add * np.eye(x.shape[1])


def run_gram(x, diag_add, tile_cols=0, rows=None, ld=None):
    """raw sbr_gram_dense into a NaN-filled guarded buffer -> the [m, m] view on the host; nothing outside [r0, r1) x [0, m) was written"""
    n, m = x.shape
    r0, r1 = (0, m) if rows is None else rows
    xt = sp.csr_matrix(x.T)
    xt.sort_indices()
    ops = [_i64(x.indptr), _i32(x.indices), _i64(xt.indptr), _i32(xt.indices)]
    out = _Buf(m, m, ld=ld or m, off=1)
    call('sbr_gram_dense', *[_p(o) for o in ops], n, m, r0, r1, float(diag_add), tile_cols, out.ptr, out.ld, _L().stream())
    return out.check_untouched(slice(r0, r1), what=f'gram rows {r0}:{r1}').contiguous().double().numpy()


@pytest.mark.parametrize('tile_cols', [0, 64])
@pytest.mark.parametrize('name', ['50x40', '300x200', '97x130'])
def test_gram_dense_is_exact(name, tile_cols):
    x = gram_matrix(name)
    m = x.shape[1]
    got = run_gram(x, 3., tile_cols, ld=m + 3 if tile_cols else m)
    assert np.array_equal(got, gram_ref(x, 3.)), f'{name} tile={tile_cols}'
    if name == '97x130':
        assert got[17, 17] == 3. and not got[17, :17].any() and not got[:, 17][18:].any()
    assert m <= 64 or tile_cols == 0 or m % 64 != 0                                # forced tiles: several, the last one ragged


def test_gram_dense_row_range_writes_only_its_rows():
    x = gram_matrix('97x130')
    ref = gram_ref(x, 500.)
    part = run_gram(x, 500., 64, rows=(30, 101))                                    # (run_gram checks that the other rows keep their NaN)
    assert np.array_equal(part[30:101], ref[30:101]) and np.isnan(part[:30]).all() and np.isnan(part[101:]).all()
    assert np.isnan(run_gram(x, 500., rows=(5, 5))).all()                           # an empty range writes nothing


def test_ops_gram_dense_and_its_errors():
    Sm = S()
    x = gram_matrix('300x200')
    csr = _feats().DeviceCSR(x).to(DEV)
    ref = gram_ref(x, 2.)
    got = Sm.ops.gram_dense(csr, 2.)
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().double().numpy(), ref)
    part = Sm.ops.gram_dense(csr, 2., rows=(64, 130), tile_cols=64)
    assert np.array_equal(part[64:130].cpu().double().numpy(), ref[64:130]) and not bool(part[:64].any()) and not bool(part[130:].any())
    big = torch.full((203, 203), SENTINEL, device=DEV)
    assert Sm.ops.gram_dense(csr, 2., out=big[:200, :200]).data_ptr() == big.data_ptr()
    assert np.array_equal(big[:200, :200].cpu().double().numpy(), ref) and bool((big[200:] == SENTINEL).all()) and bool((big[:, 200:] == SENTINEL).all())
    with pytest.raises(ValueError, match='0/1'):
        Sm.ops.gram_dense(_feats().DeviceCSR(x * 2).to(DEV))
    with pytest.raises(ValueError, match='float32'):
        Sm.ops.gram_dense(csr, out=torch.zeros(200, 200, device=DEV, dtype=torch.float64))
    with pytest.raises(Sm.SibrarHipError, match='sbr_gram_dense.*160 KiB'):
        Sm.ops.gram_dense(csr, tile_cols=50000)


# ---- sbr_spd_inverse_f32 ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inverse_case(n, lam):
    a = R.random_spd(n, lam, seed=1000 + 2 * n + lam)
    return a, np.linalg.inv(a), R.e_ref(a)


def _invert(a, padded):
    """ops.spd_inverse_ on a contiguous matrix, or on the top-left view of a larger sentinel-filled buffer (ld = n + 3) -> the view"""
    n = a.shape[0]
    a32 = torch.from_numpy(a.astype(np.float32))
    if not padded:
        return S().ops.spd_inverse_(a32.to(DEV))
    big = torch.full((n + 3, n + 3), SENTINEL, device=DEV)
    big[:n, :n] = a32.to(DEV)
    out = S().ops.spd_inverse_(big[:n, :n])
    torch.cuda.synchronize()
    assert bool((big[n:] == SENTINEL).all()) and bool((big[:, n:] == SENTINEL).all()), 'elements outside the view were written'
    return out


@pytest.mark.parametrize('lam', [1, 500])
@pytest.mark.parametrize('n', [1, 40, 64, 65, 130, 200, 257])
def test_spd_inverse(n, lam):
    a, inv, e = inverse_case(n, lam)
    got = [_invert(a, padded) for padded in (False, True, False)]
    g = got[0].cpu().double().numpy()
    err, asym = np.abs(g - inv).max(), np.abs(g - g.T).max()
    print(f'spd_inverse n={n} lam={lam}: e_ref {e:.3e} kernel err {err:.3e} ratio {err / e if e else 0.:.3f} asymmetry {asym:.3e}')
    assert err <= R.FACTOR * e, f'error {err:.3e} over 8 x e_ref = {R.FACTOR * e:.3e}'
    assert asym <= R.FACTOR * e, f'asymmetry {asym:.3e} over 8 x e_ref = {R.FACTOR * e:.3e}'
    assert torch.equal(got[1], got[0]), 'the padded view differs in bits'
    assert torch.equal(got[2], got[0]), 'a second run differs in bits'


def test_spd_inverse_reports_the_first_bad_pivot():
    Sm = S()
    d = np.ones(130, dtype=np.float32)
    d[69] = 0
    a = torch.from_numpy(np.diag(d)).to(DEV)
    ws = torch.empty(_L().lib().sbr_spd_inverse_f32_workspace(130) // 4, device=DEV)
    info = torch.zeros(1, device=DEV, dtype=torch.int32)
    call('sbr_spd_inverse_f32', _p(a), 130, 130, _p(ws), ws.numel() * 4, _p(info), _L().stream())          # returns normally
    assert int(info.item()) == 70
    with pytest.raises(ValueError, match='pivot 69'):
        Sm.ops.spd_inverse_(torch.from_numpy(np.diag(d)).to(DEV))
    ok = Sm.ops.spd_inverse_(torch.eye(5, device=DEV) * 4)                                                 # and the next call starts clean
    assert torch.equal(ok, torch.eye(5, device=DEV) / 4)


def test_spd_inverse_refuses_other_operands():
    Sm = S()
    with pytest.raises(ValueError, match='float32'):
        Sm.ops.spd_inverse_(torch.eye(4, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match='square'):
        Sm.ops.spd_inverse_(torch.ones(4, 5, device=DEV))
    with pytest.raises(ValueError, match='square'):
        Sm.ops.spd_inverse_(torch.eye(6, device=DEV).t()[::2, ::2])
    assert Sm.ops.spd_inverse_(torch.empty(0, 0, device=DEV)).shape == (0, 0)
    with pytest.raises(Sm.SibrarHipError, match='workspace'):
        call('sbr_spd_inverse_f32', _p(torch.eye(4, device=DEV)), 4, 4, None, 0, _p(torch.zeros(1, device=DEV, dtype=torch.int32)), _L().stream())


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def _inter():
    x = sp.csr_matrix(ARRAYS['inter'])
    x.sort_indices()
    return x


@functools.lru_cache(maxsize=None)
def fitted(name):
    case = next(c for c in CASES if c['name'] == name)
    return S().EASE.build_from_conf({'alg': 'ease', 'lam': case['lam']}).fit(_inter())


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_model_meets_the_reference(case):
    inter = _inter()
    m = fitted(case['name'])
    e = R.e_ref_weights(R.gram(inter, case['lam']))
    assert m.B.dtype == torch.float32 and tuple(m.B.shape) == (40, 40) and bool((m.B.diagonal() == 0).all())
    b_err = np.abs(m.B.cpu().double().numpy() - ARRAYS[case['name'] + '/B']).max()
    pred = m.predict(torch.arange(50), torch.arange(40).expand(50, 40))
    assert pred.dtype == torch.float32 and tuple(pred.shape) == (50, 40)
    rows = int(np.diff(inter.indptr).max())
    p_err = np.abs(pred.cpu().double().numpy() - ARRAYS[case['name'] + '/pred_mtx']).max()
    print(f'EASE {case["name"]}: e_ref {e:.3e} B err {b_err:.3e} ratio {b_err / e:.3f}; pred err {p_err:.3e} ratio {p_err / (e * rows):.3f}')
    assert b_err <= R.FACTOR * e and p_err <= R.FACTOR * e * rows
    full = m.combine_user_item_representations(m.get_user_representations(torch.arange(50)), m.get_item_representations(torch.arange(40)))
    assert torch.equal(full, pred)
    some = torch.tensor([31, 2, 2, 17])
    assert torch.equal(m.combine_user_item_representations(m.get_user_representations(torch.tensor([4, 4, 9])), m.get_item_representations(some)),
                       full[[4, 4, 9]][:, some.to(DEV)])


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_top10_through_evaluate_recommender_algorithm(case):
    """the users whose float64 gap between the 10th and 11th score exceeds twice the allowed score error get exactly the reference's top-10"""
    Sm = S()
    inter = _inter()
    m = fitted(case['name'])
    pred64 = ARRAYS[case['name'] + '/pred_mtx']
    counts = R.countable_users(pred64, inter, R.e_ref_weights(R.gram(inter, case['lam'])))
    assert (~counts).sum() <= R.MAX_LEFT_OUT * 50
    _, order = R.masked_topk(pred64, inter)
    rng = np.random.default_rng(23)
    lab = np.zeros((50, 40))
    for u in range(50):
        lab[u, rng.choice(np.flatnonzero(ARRAYS['inter'][u] == 0), size=3, replace=False)] = 1
    lab = sp.csr_matrix(lab)
    lab.sort_indices()
    view = SimpleNamespace(n_users=50, n_items=40, items_in_split=np.arange(40), users_in_split=np.arange(50), n_items_in_split=40,
                           n_users_in_split=50, user_sampling_matrix=lab, exclude_data=inter.astype(bool))
    ks = (5, 10)
    loader = type('L', (), {'dataset': view, 'batch_size': 16})()

    def evaluator():
        return Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=ks, metrics=('ndcg', 'recall', 'precision')), dataset=view)
    metrics, raw = Sm.evaluate_recommender_algorithm(m, loader, evaluator(), DEV, return_raw=True, user_chunk=32)
    dump = Sm.gather_recommender_algorithm_results(m, loader, evaluator(), device=DEV, user_chunk=32)
    top = np.asarray(dump['topk_item_indices'])
    assert top.shape == (50, 10) and np.array_equal(np.asarray(dump['user_indices']), np.arange(50))
    users = np.flatnonzero(counts)
    for u in users:
        assert set(top[u]) == set(order[u, :10]), f'user {u}'
    want = E.exact_recall_precision(order[users, :10], users, (lab.indptr, lab.indices), ks)
    assert np.array_equal(np.asarray(raw['recall@10'])[users], want[0, 1]) and np.array_equal(np.asarray(raw['precision@10'])[users], want[1, 1])
    assert np.array_equal(np.asarray(raw['recall@10']), np.asarray(dump['raw_metrics']['recall@10']))
    assert 0. <= metrics['ndcg@10'] <= 1.


def test_fit_300x200_meets_the_restatement():
    """more than one pivot block (200 = 3 x 64 + 8), through fit"""
    x = gram_matrix('300x200')
    for lam in (1, 50):
        g = R.gram(x, lam)
        b64, pred64 = R.fit64(x, lam)
        e = R.e_ref_weights(g)
        m = S().EASE(lam).fit(x)
        b_err = np.abs(m.B.cpu().double().numpy() - b64).max()
        u = torch.arange(0, 300, 7)
        p_err = np.abs(m.predict(u, torch.arange(200).expand(len(u), 200)).cpu().double().numpy() - pred64[u.numpy()]).max()
        rows = int(np.diff(x.indptr).max())
        print(f'EASE 300x200 lam={lam}: e_ref {e:.3e} B err {b_err:.3e} ratio {b_err / e:.3f}; pred ratio {p_err / (e * rows):.3f}')
        assert b_err <= R.FACTOR * e and p_err <= R.FACTOR * e * rows


def test_fit_is_reproducible_and_valid_in_deterministic_mode():
    Sm = S()
    x = gram_matrix('300x200')
    first = Sm.EASE(10).fit(x)
    prev = Sm.ops.set_deterministic(True)
    try:
        Sm.ops.nondeterministic_launches(reset=True)
        again = Sm.EASE(10).fit(x)
        rows = again.predict(torch.arange(300), torch.arange(200).expand(300, 200))
        torch.cuda.synchronize()
        assert Sm.ops.nondeterministic_launches(reset=True) == 0
    finally:
        Sm.ops.set_deterministic(prev)
    assert torch.equal(again.B, first.B)
    assert torch.equal(rows, first.predict(torch.arange(300), torch.arange(200).expand(300, 200)))


def test_persistence(tmp_path):
    Sm = S()
    inter = _inter()
    m = fitted('lam10')
    rng = np.random.default_rng(3)
    u = torch.from_numpy(rng.integers(0, 50, size=16))
    i = torch.from_numpy(rng.integers(0, 40, size=(16, 9)))
    got = m.predict(u, i)
    m.save_model_to_path(str(tmp_path))
    back = Sm.EASE(10)
    back.load_model_from_path(str(tmp_path))
    with pytest.raises(RuntimeError, match='attach'):
        back.predict(u, i)
    assert torch.equal(back.attach(inter).predict(u, i), got)
    other = Sm.EASE(10)
    other.load_model_from_path(str(tmp_path), matrix=inter)
    assert torch.equal(other.to(DEV).predict(u, i), got)
    with pytest.raises(ValueError, match='do not fit'):
        other.attach(gram_matrix('300x200')).predict(u, i)
