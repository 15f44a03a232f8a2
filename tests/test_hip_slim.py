"""csrc/slim.hip on the GPU: sbr_slim_cd_f32 against the float64 restatement of tests/slim_ref.py, with the distance of the float32 run
of the same loop from it as the yardstick — e_ref = max |cd_float32 - cd_float64| at the same max_iter and tol = 0, so that both sides run the
same sweeps; kernel error <= 8 e_ref, the margin of tests/test_hip_ease.py — and SLIM against the g26 fixture recorded from the reference,
through evaluate_recommender_algorithm, in deterministic mode and through model.npz. Every ratio is printed before it is asserted."""
import functools
import importlib
import logging
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import evalk_ref as E
import slim_ref as R
from hip_testutil import DEV, S, _Buf, _L, call

pytestmark = pytest.mark.gpu

ARRAYS, CASES = R.load_g26()
IDS = [c['name'] for c in CASES]
SWEEPS = 30                                  # max_iter of the yardstick runs (tol = 0: every column runs them all, or ends at a fixed point)
PARAMS5 = tuple((a, l) for a, l, _ in R.PARAMS) + ((0.02, 0.), (0.02, 1.))
EMPTY, TWINS = 7, (3, 30)                    # of the 70x45 world: an item nobody holds, two identical item columns


def _feats():
    return importlib.import_module(S().ops.__name__.rsplit('.', 1)[0] + '.features')


@functools.lru_cache(maxsize=None)
def matrix(name):
    """users x items, 0/1, csr float64"""
    if name == '50x40':
        x = sp.csr_matrix(ARRAYS['inter'])
        x.sort_indices()
        return x
    if name == '70x45':
        return R.world(70, 45, 0.12, seed=5, empty_item=EMPTY, twin=TWINS)
    n, m = (int(v) for v in name.split('x'))
    if m > 1024:                                                   # more than one chunk of 1,024 coordinates: the last item is a copy of item 10
        return R.world(n, m, 0.1 + 0.05 * (m % 2), seed=n + m, twin=(10, m - 1))
    return R.world(n, m, 0.6 if m <= 2 else 0.1 + 0.05 * (m % 2), seed=n + m)          # 0.1 or 0.15; the two tiny ones need some entries


@functools.lru_cache(maxsize=None)
def gram(name):
    return R.gram(matrix(name))


@functools.lru_cache(maxsize=None)
def yardstick(name, alpha, l1_ratio, max_iter=SWEEPS, cols=None):
    """(l1, l2, e_ref, W float64, W float32) at tol = 0; ``cols``: a tuple of target columns (None: all)"""
    l1, l2 = R.penalties(matrix(name).shape[0], alpha, l1_ratio)
    return (l1, l2) + R.e_ref(gram(name), l1, l2, max_iter, cols)


def run(name, l1, l2, max_iter, tol, cols=None, padded=False, w_buf=None):
    """raw sbr_slim_cd_f32 on the world's Gram matrix -> (W buffer, n_iter on the host); ``padded``: G and W as views with ld = m + 3
    inside NaN-guarded buffers. n_iter holds -77 where it was not written."""
    g = torch.from_numpy(gram(name).astype(np.float32))
    m = g.shape[0]
    c0, c1 = (0, m) if cols is None else cols
    gb = _Buf(m, m, ld=m + 3 if padded else m, off=1 if padded else 0, data=g)
    wb = w_buf or _Buf(m, m, ld=m + 3 if padded else m, off=3 if padded else 0)
    n_iter = torch.full((m,), -77, device=DEV, dtype=torch.int32)
    call('sbr_slim_cd_f32', gb.ptr, m, gb.ld, c0, c1, float(l1), float(l2), int(max_iter), float(tol), wb.ptr, wb.ld, n_iter.data_ptr(),
         _L().stream())
    assert torch.equal(gb.check_untouched(None, what='G'), g), 'G was written'
    return wb, n_iter.cpu().numpy()


def columns(wb, c0, c1):
    """the view on the host, after checking that only columns [c0, c1) of it (and nothing around it) were written"""
    host = wb.check_untouched(None, what='W')
    assert torch.isnan(host[:, :c0]).all() and torch.isnan(host[:, c1:]).all(), 'columns outside the range were written'
    assert not torch.isnan(host[:, c0:c1]).any(), 'an element of an owned column was not written'
    return host[:, c0:c1].contiguous()


SHAPES = ['3x1', '4x2', '50x40', '90x63', '90x64', '90x65', '300x257', '300x200']


@pytest.mark.parametrize('name, alpha, l1_ratio', [(n, 0.01, 0.5) for n in SHAPES] + [(n, a, l) for n in ('50x40', '90x65') for a, l in PARAMS5[1:]])
def test_kernel_meets_the_restatement(name, alpha, l1_ratio):
    l1, l2, e, w64, w32 = yardstick(name, alpha, l1_ratio)
    m = w64.shape[0]
    wb, n_iter = run(name, l1, l2, SWEEPS, 0.)
    w = columns(wb, 0, m)
    err = float(np.abs(w.double().numpy() - w64).max())
    same = bool(np.array_equal(w.numpy(), w32))
    print(f'slim {name} alpha={alpha} l1_ratio={l1_ratio}: e_ref {e:.3e} kernel err {err:.3e} ratio {err / e if e else 0.:.3f} '
          f'(the float32 restatement bit for bit: {same}); nnz/col {float((w > 0).sum()) / m:.1f}; sweeps {np.abs(n_iter).max()}')
    assert err <= R.FACTOR * e, f'error {err:.3e} over 8 x e_ref = {R.FACTOR * e:.3e}'
    assert bool((w >= 0).all()) and not bool(w.diagonal().any())
    assert ((n_iter == -SWEEPS) | ((n_iter >= 1) & (n_iter <= SWEEPS))).all()


# Catalogues of more than 1,024 items: a column is walked in several chunks of 1,024 coordinates (a thread owns several of them, one bit
# each), and above 4,096 items a thread's elements of a row of G are no longer all loaded before the step is known. A few target columns
# per size, in different chunks and at chunk edges, so that the numpy restatement stays within a second.
BIG = {'200x1025': ((8, 12), (1022, 1025)),
       '200x2100': ((8, 12), (1022, 1026), (2097, 2100)),
       '200x4100': ((8, 12), (1023, 1025), (3000, 3002), (4095, 4100))}


@pytest.mark.parametrize('name', list(BIG))
def test_more_than_one_chunk_meets_the_restatement(name):
    ranges = BIG[name]
    cols = tuple(j for c0, c1 in ranges for j in range(c0, c1))
    l1, l2, e, w64, w32 = yardstick(name, 0.01, 0.5, SWEEPS, cols)
    m = w64.shape[0]
    assert e > 0 and 10 in cols and m - 1 in cols
    got = []
    for c0, c1 in ranges:
        wb, n_iter = run(name, l1, l2, SWEEPS, 0., cols=(c0, c1))
        got.append(columns(wb, c0, c1))
        assert (n_iter[:c0] == -77).all() and (n_iter[c1:] == -77).all() and (n_iter[c0:c1] != -77).all()
    w = torch.cat(got, dim=1)
    err = float(np.abs(w.double().numpy() - w64).max())
    beyond = [int((w[lo:] > 0).sum()) for lo in range(1024, m, 1024)]
    print(f'slim {name} columns {ranges}: e_ref {e:.3e} kernel err {err:.3e} ratio {err / e:.3f} (the float32 restatement bit for bit: '
          f'{bool(np.array_equal(w.numpy(), w32))}); non-zero weights from coordinate 1024, 2048, ... on: {beyond}')
    assert err <= R.FACTOR * e, f'error {err:.3e} over 8 x e_ref = {R.FACTOR * e:.3e}'
    assert bool((w >= 0).all()) and all(float(w[j, i]) == 0 for i, j in enumerate(cols))
    assert all(b > 0 for b in beyond), 'no weight in one of the later chunks: the case does not reach it'
    # the twins name each other across the chunks: item 10 (chunk 0) and the last item (the last chunk)
    assert float(w[m - 1, cols.index(10)]) > 0.3 and float(w[10, cols.index(m - 1)]) > 0.3


def test_more_than_one_chunk_splits_and_views_agree_in_bits():
    name, m, c0, c1 = '200x2100', 2100, 1020, 1030                 # targets on both sides of the first chunk edge
    l1, l2 = R.penalties(200, 0.01, 0.5)
    wb, it = run(name, l1, l2, 500, R.TOL, cols=(c0, c1))
    w = columns(wb, c0, c1)
    assert int((w[1024:] > 0).sum()) > 0 and int((w[:1024] > 0).sum()) > 0
    for padded in (False, True):
        parts, iters = [], []
        for a, b in ((c0, 1024), (1024, c1)):
            pb, ni = run(name, l1, l2, 500, R.TOL, cols=(a, b), padded=padded)
            parts.append(columns(pb, a, b))
            iters.append(ni[a:b])
        assert torch.equal(torch.cat(parts, dim=1), w), f'the splits differ in bits (padded={padded})'
        assert np.array_equal(np.concatenate(iters), it[c0:c1])
    pb, ni = run(name, l1, l2, 500, R.TOL, cols=(c0, c1), padded=True)
    assert torch.equal(columns(pb, c0, c1), w) and np.array_equal(ni, it), 'the padded views differ in bits'
    assert torch.equal(columns(run(name, l1, l2, 500, R.TOL, cols=(c0, c1))[0], c0, c1), w), 'a second run differs in bits'


def test_runs_splits_and_views_agree_in_bits():
    name = '90x65'
    l1, l2 = R.penalties(90, 0.01, 0.5)
    m = 65
    whole, it = run(name, l1, l2, 500, R.TOL)
    w = columns(whole, 0, m)
    again = columns(run(name, l1, l2, 500, R.TOL)[0], 0, m)
    assert torch.equal(again, w), 'a second run differs in bits'
    for padded in (False, True):
        parts, iters = [], []
        for c0, c1 in ((0, 1), (1, 33), (33, m)):
            wb, ni = run(name, l1, l2, 500, R.TOL, cols=(c0, c1), padded=padded)
            parts.append(columns(wb, c0, c1))
            assert (ni[:c0] == -77).all() and (ni[c1:] == -77).all()
            iters.append(ni[c0:c1])
        assert torch.equal(torch.cat(parts, dim=1), w), f'the splits differ in bits (padded={padded})'
        assert np.array_equal(np.concatenate(iters), it)
    wb, ni = run(name, l1, l2, 500, R.TOL, padded=True)
    assert torch.equal(columns(wb, 0, m), w) and np.array_equal(ni, it), 'the padded views differ in bits'
    wb, ni = run(name, l1, l2, 500, R.TOL, cols=(9, 9))                                # an empty range writes nothing
    assert torch.isnan(wb.check_untouched(None)).all() and (ni == -77).all()
    assert (it >= 1).all() and it.max() < 500


def test_kkt_residual_at_the_default_tolerance():
    for name, n in (('50x40', 50), ('300x200', 300)):
        g = gram(name)
        for alpha, l1_ratio in PARAMS5[:3] if name == '50x40' else PARAMS5[:1]:
            l1, l2 = R.penalties(n, alpha, l1_ratio)
            w32, it32, _ = R.cd(g, l1, l2, 500, R.TOL, np.float32)
            want = R.kkt_all(g, w32, l1, l2)
            wb, it = run(name, l1, l2, 500, R.TOL)
            w = columns(wb, 0, g.shape[0]).double().numpy()
            got = R.kkt_all(g, w, l1, l2)
            print(f'slim KKT {name} alpha={alpha} l1_ratio={l1_ratio}: float32 restatement {want:.3e} kernel {got:.3e} ratio {got / want if want else 0.:.3f}; '
                  f'sweeps kernel <= {it.max()} restatement <= {it32.max()}')
            assert got <= R.FACTOR * want and (it >= 1).all()


def test_edges():
    name, n, m = '70x45', 70, 45
    g = gram(name)
    assert g[EMPTY, EMPTY] == 0 and np.array_equal(g[TWINS[0]], g[TWINS[1]])
    l1, l2, e, w64, _ = yardstick(name, 0.01, 0.5)
    w = columns(run(name, l1, l2, SWEEPS, 0.)[0], 0, m)
    assert float(np.abs(w.double().numpy() - w64).max()) <= R.FACTOR * e
    assert not bool(w[EMPTY].any()) and not bool(w[:, EMPTY].any()), 'an item nobody holds: its row and its column are zero'
    assert float(w[TWINS[1], TWINS[0]]) > 0.3 and float(w[TWINS[0], TWINS[1]]) > 0.3, 'identical items name each other'
    # an l1 above every entry of G: no coordinate can move, one sweep finds that out
    wb, it = run(name, float(g.max()) + 1., l2, 500, R.TOL)
    assert not bool(columns(wb, 0, m).any()) and (it == 1).all()
    # max_iter = 1: a column with a non-zero step cannot have met the stopping test
    _, _, steps = R.cd(g, l1, l2, 1, R.TOL, np.float32)
    wb, it = run(name, l1, l2, 1, R.TOL)
    columns(wb, 0, m)
    assert np.array_equal(it, np.where(steps > 0, -1, 1)) and steps[EMPTY] == 0 and (steps > 0).any()


def test_ops_slim_weights_and_its_errors():
    Sm = S()
    l1, l2, e, w64, _ = yardstick('90x65', 0.01, 0.5)
    g = torch.from_numpy(gram('90x65').astype(np.float32)).to(DEV)
    w, it = Sm.ops.slim_weights(g, l1, l2, SWEEPS, tol=0.)
    assert w.dtype == torch.float32 and it.dtype == torch.int32 and tuple(w.shape) == (65, 65) and tuple(it.shape) == (65,)
    assert float(np.abs(w.cpu().double().numpy() - w64).max()) <= R.FACTOR * e
    part, pit = Sm.ops.slim_weights(g, l1, l2, SWEEPS, tol=0., cols=(10, 40))
    assert torch.equal(part[:, 10:40], w[:, 10:40]) and not bool(part[:, :10].any()) and not bool(part[:, 40:].any())
    assert torch.equal(pit[10:40], it[10:40]) and not bool(pit[:10].any()) and not bool(pit[40:].any())
    big = torch.full((68, 68), 7.25, device=DEV)
    big[:65, :65] = g
    out = torch.full((68, 68), 7.25, device=DEV)
    assert Sm.ops.slim_weights(big[:65, :65], l1, l2, SWEEPS, tol=0., out=out[:65, :65])[0].data_ptr() == out.data_ptr()
    assert torch.equal(out[:65, :65], w) and bool((out[65:] == 7.25).all()) and bool((out[:, 65:] == 7.25).all())
    assert tuple(Sm.ops.slim_weights(torch.empty(0, 0, device=DEV), 1., 1., 3)[0].shape) == (0, 0)
    with pytest.raises(ValueError, match='float32'):
        Sm.ops.slim_weights(g.double(), l1, l2, 5)
    with pytest.raises(ValueError, match='square'):
        Sm.ops.slim_weights(g[:, :60], l1, l2, 5)
    with pytest.raises(ValueError, match='negative'):
        Sm.ops.slim_weights(g, -1., l2, 5)
    with pytest.raises(ValueError, match='max_iter'):
        Sm.ops.slim_weights(g, l1, l2, 0)
    with pytest.raises(Sm.SibrarHipError, match='column range'):
        Sm.ops.slim_weights(g, l1, l2, 5, cols=(60, 66))
    for gm, out in ((g, g), (big[:65, :65], big[:65, :65]), (big[:65, :65], big[3:68, :65]), (big[3:68, 3:68], big[:65, :65])):
        with pytest.raises(ValueError, match='overlaps'):
            Sm.ops.slim_weights(gm, l1, l2, 5, out=out)
    apart = torch.zeros(2 * 65 * 65, device=DEV)                   # G and out back to back in one allocation do not overlap
    apart[:65 * 65] = g.reshape(-1)
    w2, _ = Sm.ops.slim_weights(apart[:65 * 65].view(65, 65), l1, l2, SWEEPS, tol=0., out=apart[65 * 65:].view(65, 65))
    assert torch.equal(w2, w)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fitted(name):
    """the fixture's case at tol = 0: the sweeps of ``yardstick('50x40', ..., max_iter)``"""
    case = next(c for c in CASES if c['name'] == name)
    return S().SLIM(case['alpha'], case['l1_ratio'], case['max_iter'], tol=0.).fit(matrix('50x40'))


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_model_meets_the_optimum(case):
    inter = matrix('50x40')
    m = fitted(case['name'])
    _, _, e, w64, _ = yardstick('50x40', case['alpha'], case['l1_ratio'], case['max_iter'])
    w_opt = ARRAYS[case['name'] + '/W_opt']
    rest = float(np.abs(w64 - w_opt).max())                  # the float64 restatement at tol = 0 against the one at tol = 1e-12
    assert m.W.dtype == torch.float32 and tuple(m.W.shape) == (40, 40) and bool((m.W.diagonal() == 0).all()) and bool((m.W >= 0).all())
    w = m.W.cpu().double().numpy()
    err, err_opt = float(np.abs(w - w64).max()), float(np.abs(w - w_opt).max())
    pred = m.predict(torch.arange(50), torch.arange(40).expand(50, 40))
    assert pred.dtype == torch.float32 and tuple(pred.shape) == (50, 40)
    rows = int(np.diff(inter.indptr).max())
    p_err = float(np.abs(pred.cpu().double().numpy() - np.asarray(inter @ w_opt)).max())
    print(f'SLIM {case["name"]}: e_ref {e:.3e} W err {err:.3e} ratio {err / e:.3f}; against W_opt {err_opt:.3e} (restatements apart {rest:.3e}); '
          f'score err {p_err:.3e} ratio {p_err / (e * rows):.3f}; sweeps <= {int(m.n_iter_.abs().max())}')
    assert rest <= 1e-9 and err <= R.FACTOR * e and err_opt <= R.FACTOR * e + rest and p_err <= (R.FACTOR * e + rest) * rows
    full = m.combine_user_item_representations(m.get_user_representations(torch.arange(50)), m.get_item_representations(torch.arange(40)))
    assert torch.equal(full, pred)
    some = torch.tensor([31, 2, 2, 17])
    assert torch.equal(m.combine_user_item_representations(m.get_user_representations(torch.tensor([4, 4, 9])), m.get_item_representations(some)),
                       full[[4, 4, 9]][:, some.to(DEV)])
    rng = np.random.default_rng(3)
    u, i = torch.from_numpy(rng.integers(0, 50, size=16)), torch.from_numpy(rng.integers(0, 40, size=(16, 9)))
    assert torch.equal(m.predict(u, i), torch.gather(full[u.to(DEV)], 1, i.to(DEV))), 'predict is a selection of the same rows'


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_top10_through_evaluate_recommender_algorithm(case):
    """every countable user (tests/slim_ref.py's rule) gets exactly the top-10 of the reference's pred_mtx"""
    Sm = S()
    inter = matrix('50x40')
    m = fitted(case['name'])
    pred_ref = ARRAYS[case['name'] + '/pred_mtx']
    e = yardstick('50x40', case['alpha'], case['l1_ratio'], case['max_iter'])[2]
    counts = R.countable_users(pred_ref, np.asarray(inter @ ARRAYS[case['name'] + '/W_opt']), inter, R.FACTOR * e)
    assert (~counts).sum() <= R.MAX_LEFT_OUT * 50
    _, order = R.masked_topk(pred_ref, inter)
    rng = np.random.default_rng(26)
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
    print(f'SLIM {case["name"]}: {len(users)} of 50 users compared')
    for u in users:
        assert set(top[u]) == set(order[u, :10]), f'user {u}'
    want = E.exact_recall_precision(order[users, :10], users, (lab.indptr, lab.indices), ks)
    assert np.array_equal(np.asarray(raw['recall@10'])[users], want[0, 1]) and np.array_equal(np.asarray(raw['precision@10'])[users], want[1, 1])
    assert 0. <= metrics['ndcg@10'] <= 1.


def test_fit_is_reproducible_valid_in_deterministic_mode_and_warns(caplog):
    Sm = S()
    x = matrix('300x200')
    first = Sm.SLIM(0.01, 0.5, 100).fit(x)
    assert first.n_iter_.dtype == torch.int32 and bool((first.n_iter_ >= 1).all())
    prev = Sm.ops.set_deterministic(True)
    try:
        Sm.ops.nondeterministic_launches(reset=True)
        again = Sm.SLIM(0.01, 0.5, 100).fit(x)
        rows = again.predict(torch.arange(300), torch.arange(200).expand(300, 200))
        torch.cuda.synchronize()
        assert Sm.ops.nondeterministic_launches(reset=True) == 0
    finally:
        Sm.ops.set_deterministic(prev)
    assert torch.equal(again.W, first.W) and torch.equal(again.n_iter_, first.n_iter_)
    assert torch.equal(rows, first.predict(torch.arange(300), torch.arange(200).expand(300, 200)))
    with caplog.at_level(logging.WARNING):
        caplog.clear()
        late = Sm.SLIM(0.01, 0.5, 1).fit(x)
    n_late = int((late.n_iter_ < 0).sum())
    assert n_late > 0 and any(f'{n_late} of 200 columns did not converge' in r.getMessage() for r in caplog.records)
    with caplog.at_level(logging.WARNING):
        caplog.clear()
        Sm.SLIM(0.01, 0.5, 100).fit(x)
    assert not any('did not converge' in r.getMessage() for r in caplog.records)


def test_persistence(tmp_path):
    Sm = S()
    inter = matrix('50x40')
    m = fitted(IDS[0])
    rng = np.random.default_rng(3)
    u = torch.from_numpy(rng.integers(0, 50, size=16))
    i = torch.from_numpy(rng.integers(0, 40, size=(16, 9)))
    got = m.predict(u, i)
    m.save_model_to_path(str(tmp_path))
    back = Sm.SLIM(0.5, 0.5, 1)
    back.load_model_from_path(str(tmp_path))
    with pytest.raises(RuntimeError, match='attach'):
        back.predict(u, i)
    assert torch.equal(back.attach(inter).predict(u, i), got)
    other = Sm.SLIM(0.5, 0.5, 1)
    other.load_model_from_path(str(tmp_path), matrix=inter)
    assert torch.equal(other.to(DEV).predict(u, i), got)
    with pytest.raises(ValueError, match='do not fit'):
        other.attach(matrix('300x200')).predict(u, i)
