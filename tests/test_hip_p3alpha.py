"""csrc/p3alpha.hip on the GPU: sbr_p3_walk_dense and sbr_p3_score_rows (alpha = 1) bit for bit against the fp32 order oracle of
tests/p3alpha_ref.py, the power against float64 pow of the oracle's pre-power value to 16 ulp, and P3alpha against the g24 fixture recorded
from the reference: elementwise within the derived bound, the top-10 through evaluate_recommender_algorithm, in deterministic mode and
through model.npz. Every measured figure is printed before it is asserted."""
import functools
import importlib
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import evalk_ref as E
import p3alpha_ref as R
from hip_testutil import DEV, S, _Buf, _i32, _i64, _L, _p, call

pytestmark = pytest.mark.gpu

ARRAYS, CASES = R.load_g24()
IDS = [c['name'] for c in CASES]
SENTINEL = 7.25
WORLDS = ['50x40', '300x200', '97x130']


def _feats():
    return importlib.import_module(S().ops.__name__.rsplit('.', 1)[0] + '.features')


@functools.lru_cache(maxsize=None)
def world(name):
    """(X, the oracle's W as float32 numpy) — computed once, never changed"""
    if name == '40x1100':
        # beyond the issue's worlds: more than 1,024 columns (two column blocks of the score rows) and, at the default tile, strips
        # of 69 columns, which the user holding every item crosses in two passes of the wave
        d = np.random.default_rng(1140).random((40, 1100)) < 0.05
        d[3], d[:, 5], d[38], d[:, 1097] = True, True, False, False
        x = sp.csr_matrix(d.astype(np.float64))
        x.sort_indices()
    else:
        x = R.world(name, ARRAYS['inter'])
    w = R.walk32(x)
    return x, w


def _csr_ops(x):
    xt = sp.csr_matrix(x.T)
    xt.sort_indices()
    return [_i64(x.indptr), _i32(x.indices), _i64(xt.indptr), _i32(xt.indices)]


def run_walk(x, tile_cols=0, rows=None, ld=None):
    """raw sbr_p3_walk_dense into a NaN-filled guarded buffer -> the [m, m] view on the host; nothing outside [r0, r1) x [0, m) was written"""
    n, m = x.shape
    r0, r1 = (0, m) if rows is None else rows
    ops = _csr_ops(x)
    out = _Buf(m, m, ld=ld or m, off=1)
    call('sbr_p3_walk_dense', *[_p(o) for o in ops], n, m, r0, r1, tile_cols, out.ptr, out.ld, _L().stream())
    return out.check_untouched(slice(r0, r1), what=f'walk rows {r0}:{r1}').contiguous()


# ---- sbr_p3_walk_dense ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tile_cols', [0, 64])
@pytest.mark.parametrize('name', WORLDS + ['40x1100'])
def test_walk_equals_the_order_oracle(name, tile_cols):
    x, w = world(name)
    n, m = x.shape
    got = run_walk(x, tile_cols, ld=m + 3 if tile_cols else m)
    assert got.dtype == torch.float32 and torch.equal(got, torch.from_numpy(w)), f'{name} tile={tile_cols}'
    empty_item = 1097 if name == '40x1100' else m - 3
    assert not bool(got[empty_item].any()) and not bool(got[:, empty_item].any())          # zeros, not NaN
    assert m <= 64 or tile_cols == 0 or m % 64 != 0                                        # forced tiles: several, the last one ragged
    assert torch.equal(run_walk(x, tile_cols), got), 'a second run differs in bits'


def test_walk_row_range_writes_only_its_rows():
    x, w = world('97x130')
    ref = torch.from_numpy(w)
    part = run_walk(x, 64, rows=(30, 101))                                                # (run_walk checks that the other rows keep their NaN)
    assert torch.equal(part[30:101], ref[30:101]) and bool(torch.isnan(part[:30]).all()) and bool(torch.isnan(part[101:]).all())
    assert bool(torch.isnan(run_walk(x, rows=(5, 5))).all())                              # an empty range writes nothing
    one = run_walk(x, rows=(127, 128), ld=133)                                            # the empty item's row alone: written, as zeros
    assert not bool(one[127].any()) and bool(torch.isnan(one[:127]).all())


def test_ops_walk_dense_out_views_and_errors():
    Sm = S()
    x, w = world('300x200')
    ref = torch.from_numpy(w).to(DEV)
    csr = _feats().DeviceCSR(x).to(DEV)
    got = Sm.ops.p3_walk_dense(csr)
    assert got.dtype == torch.float32 and torch.equal(got, ref)
    part = Sm.ops.p3_walk_dense(csr, rows=(64, 130), tile_cols=64)
    assert torch.equal(part[64:130], ref[64:130]) and not bool(part[:64].any()) and not bool(part[130:].any())
    big = torch.full((203, 203), SENTINEL, device=DEV)                                    # a strided view of a sentinel-filled buffer
    assert Sm.ops.p3_walk_dense(csr, rows=(10, 150), out=big[:200, :200]).data_ptr() == big.data_ptr()
    assert torch.equal(big[10:150, :200], ref[10:150])
    keep = torch.ones(203, 203, dtype=torch.bool, device=DEV)
    keep[10:150, :200] = False
    assert bool((big[keep] == SENTINEL).all()), 'bytes outside the owned rows were written'
    with pytest.raises(ValueError, match='0/1'):
        Sm.ops.p3_walk_dense(_feats().DeviceCSR(x * 2).to(DEV))
    with pytest.raises(ValueError, match='float32'):
        Sm.ops.p3_walk_dense(csr, out=torch.zeros(200, 200, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match='unit column stride'):
        Sm.ops.p3_walk_dense(csr, out=torch.zeros(200, 400, device=DEV)[:, ::2])
    with pytest.raises(Sm.SibrarHipError, match='sbr_p3_walk_dense.*160 KiB'):
        Sm.ops.p3_walk_dense(csr, tile_cols=50000)
    with pytest.raises(Sm.SibrarHipError, match='sbr_p3_walk_dense.*row range'):
        Sm.ops.p3_walk_dense(csr, rows=(100, 201))


# ---- sbr_p3_score_rows ------------------------------------------------------------------------------------------------------------------
def _rows_for(x):
    """a rows tensor with a duplicate, the empty user and the user holding every item, in no order"""
    n = x.shape[0]
    empty = int(np.flatnonzero(np.diff(x.indptr) == 0)[0])
    return np.array([7, empty, 3, 0, 7, n - 1, empty, 12])


@pytest.mark.parametrize('name', WORLDS + ['40x1100'])
def test_score_rows_at_alpha_one_equal_the_order_oracle(name):
    x, w = world(name)
    n, m = x.shape
    csr = _feats().DeviceCSR(x).to(DEV)
    wd = torch.from_numpy(w).to(DEV)
    rows = _rows_for(x)
    got = S().ops.p3_score_rows(csr, torch.from_numpy(rows).to(DEV), wd, 1.0)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(rows), m)
    assert torch.equal(got.cpu(), torch.from_numpy(R.pre_power32(x, w, rows))), name
    assert not bool(got[1].any()) and torch.equal(got[0], got[4])                          # the empty user; the duplicate
    full = S().ops.p3_score_rows(csr, None, wd, 1.0)
    assert tuple(full.shape) == (n, m) and torch.equal(full.cpu(), torch.from_numpy(R.pre_power32(x, w)))
    # a strided out and W (leading dimensions beyond m), through the raw entry point: nothing outside the rows' [0, m) is written
    out = _Buf(len(rows), m, ld=m + 5, off=1)
    wb = _Buf(m, m, ld=m + 3, off=1, data=torch.from_numpy(w))
    call('sbr_p3_score_rows', _p(csr.indptr), _p(csr.indices), _p(_i64(rows)), len(rows), wb.ptr, wb.ld, m, 1.0, out.ptr, out.ld, _L().stream())
    assert torch.equal(out.check_untouched(what='score rows').contiguous(), got.cpu())


@pytest.mark.parametrize('alpha', [1.9, 0.5])
@pytest.mark.parametrize('name', WORLDS)
def test_score_rows_power_within_16_ulp(name, alpha):
    x, w = world(name)
    csr = _feats().DeviceCSR(x).to(DEV)
    got = S().ops.p3_score_rows(csr, None, torch.from_numpy(w).to(DEV), alpha).cpu().double().numpy()
    ref = R.power64(R.pre_power32(x, w), alpha)                                            # float64 pow of the bit-known fp32 value
    ulps = np.abs(got - ref) / R.ulp32(ref)
    print(f'P3alpha pow {name} alpha={alpha}: max error {ulps[ref > 0].max():.3f} ulp over {int((ref > 0).sum())} values')
    assert np.array_equal(got == 0, ref == 0), 'a zero must stay a zero'
    assert (ulps[ref > 0] <= R.POW_ULP).all()


def test_ops_score_rows_errors():
    Sm = S()
    x, w = world('50x40')
    csr = _feats().DeviceCSR(x).to(DEV)
    wd = torch.from_numpy(w).to(DEV)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Sm.ops.p3_score_rows(csr, torch.tensor([0]), wd, 1.)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Sm.ops.p3_score_rows(csr, None, torch.from_numpy(w), 1.)
    with pytest.raises(ValueError, match='contiguous float32'):
        Sm.ops.p3_score_rows(csr, None, wd.t(), 1.)
    with pytest.raises(ValueError, match='must be positive'):
        Sm.ops.p3_score_rows(csr, None, wd, 0.)
    assert tuple(Sm.ops.p3_score_rows(csr, torch.empty(0, dtype=torch.long, device=DEV), wd, 1.9).shape) == (0, 40)
    with pytest.raises(Sm.SibrarHipError, match='sbr_p3_score_rows.*alpha'):
        call('sbr_p3_score_rows', _p(csr.indptr), _p(csr.indices), None, 50, _p(wd), 40, 40, float('inf'), _p(torch.empty(50, 40, device=DEV)), 40,
             _L().stream())


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def _inter(case):
    x = sp.csr_matrix(ARRAYS[case['matrix']])
    x.sort_indices()
    return x


@functools.lru_cache(maxsize=None)
def fitted(name):
    case = next(c for c in CASES if c['name'] == name)
    return S().P3alpha.build_from_conf({'alg': 'p3alpha', 'alpha': case['alpha']}).fit(_inter(case))


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_model_meets_the_reference(case):
    inter, ref = _inter(case), ARRAYS[case['name'] + '/pred_mtx']
    m = fitted(case['name'])
    assert m.W.dtype == torch.float32 and tuple(m.W.shape) == (40, 40)
    assert torch.equal(m.W.cpu(), torch.from_numpy(R.walk32(inter)))
    pred = m.predict(torch.arange(50), torch.arange(40).expand(50, 40))
    assert pred.dtype == torch.float32 and tuple(pred.shape) == (50, 40)
    got = pred.cpu().double().numpy()
    bound = R.rel_bound(inter, case['alpha']) * ref
    err = np.abs(got - ref)
    print(f'P3alpha {case["name"]}: worst error / bound {float((err[ref > 0] / bound[ref > 0]).max()):.3f}')
    assert np.array_equal(got == 0, ref == 0), 'exact zeros of the reference must be exact zeros'
    assert (err <= bound).all()
    full = m.combine_user_item_representations(m.get_user_representations(torch.arange(50)), m.get_item_representations(torch.arange(40)))
    assert torch.equal(full, pred)
    some = torch.tensor([31, 2, 2, 17])
    assert torch.equal(m.combine_user_item_representations(m.get_user_representations(torch.tensor([4, 4, 9])), m.get_item_representations(some)),
                       full[[4, 4, 9]][:, some.to(DEV)])


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_top10_through_evaluate_recommender_algorithm(case):
    """the users the near-tie rule counts (all but those the maker recorded) get exactly the reference's top-10"""
    Sm = S()
    inter = _inter(case)
    m = fitted(case['name'])
    pred64 = ARRAYS[case['name'] + '/pred_mtx']
    counts = R.countable_users(pred64, inter, case['alpha'])
    assert int((~counts).sum()) == case['users_left_out'] <= R.MAX_LEFT_OUT * 50
    _, order = R.masked_topk(pred64, inter)
    rng = np.random.default_rng(24)
    lab = np.zeros((50, 40))
    for u in range(50):
        lab[u, rng.choice(np.flatnonzero(ARRAYS[case['matrix']][u] == 0), size=3, replace=False)] = 1
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


def test_fit_is_reproducible_and_valid_in_deterministic_mode():
    Sm = S()
    x, w = world('300x200')
    everyone = (torch.arange(300), torch.arange(200).expand(300, 200))
    first = Sm.P3alpha(1.9).fit(x)
    second = Sm.P3alpha(1.9).fit(x)
    assert torch.equal(second.W, first.W) and torch.equal(first.W.cpu(), torch.from_numpy(w))
    before = Sm.ops.nondeterministic_launches()
    prev = Sm.ops.set_deterministic(True)
    try:
        again = Sm.P3alpha(1.9).fit(x)
        rows = again.predict(*everyone)
        torch.cuda.synchronize()
        assert Sm.ops.nondeterministic_launches() == before
    finally:
        Sm.ops.set_deterministic(prev)
    assert torch.equal(again.W, first.W)
    assert torch.equal(rows, first.predict(*everyone))


def test_persistence(tmp_path):
    Sm = S()
    case = CASES[0]
    inter = _inter(case)
    m = fitted(case['name'])
    rng = np.random.default_rng(3)
    u = torch.from_numpy(rng.integers(0, 50, size=16))
    i = torch.from_numpy(rng.integers(0, 40, size=(16, 9)))
    got = m.predict(u, i)
    m.save_model_to_path(str(tmp_path))
    back = Sm.P3alpha(case['alpha'])
    back.load_model_from_path(str(tmp_path))
    with pytest.raises(RuntimeError, match='attach'):
        back.predict(u, i)
    assert torch.equal(back.attach(inter).predict(u, i), got)
    other = Sm.P3alpha(case['alpha'])
    other.load_model_from_path(str(tmp_path), matrix=inter)
    assert torch.equal(other.to(DEV).predict(u, i), got)
    with pytest.raises(ValueError, match='do not fit'):
        other.attach(world('300x200')[0]).predict(u, i)
