"""csrc/als.hip on the GPU: sbr_als_gram_f32 against float64 within the bound of a sum of n terms, sbr_als_solve_rows_f32 against the
float64 system of every row with the backward error of the plain fp32 solve of tests/als_ref.py as the yardstick (kernel <= 8 x
yardstick: another fixed summation order and an unblocked factorisation carry errors of the same size, not the same value), the error
returns, and AlternatingLeastSquare through fit, the hooks and evaluate_recommender_algorithm. Every figure is printed before it is asserted."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import als_ref as R
from hip_testutil import DEV, S, U32, _Buf, _assert_bits, _assert_bound, _i32, _i64, _L, _p, call

pytestmark = pytest.mark.gpu


# ---- sbr_als_gram_f32 -------------------------------------------------------------------------------------------------------------------
def run_gram(y, reg, ldy, ldg):
    n, f = y.shape
    yb = _Buf(n, f, ld=ldy, off=1, data=torch.from_numpy(y))
    g = _Buf(f, f, ld=ldg, off=1)
    need = int(_L().lib().sbr_als_gram_f32_workspace(n, f))
    ws = torch.empty(max(need // 4, 1), device=DEV)
    call('sbr_als_gram_f32', yb.ptr, n, yb.ld, f, float(reg), g.ptr, g.ld, _p(ws), need, _L().stream())
    return g.check_untouched(what=f'gram {n}x{f}').contiguous()


@pytest.mark.parametrize('n,f', [(1, 1), (130, 7), (700, 65), (3000, 128)])
def test_gram(n, f):
    y = R.uniform_factors(n, f, seed=n + f) * np.float32(f)                        # uniform(-0.5, 0.5): the bound is relative anyway
    reg = 0.01
    got = run_gram(y, reg, ldy=f + 3, ldg=f + 5)
    g64 = torch.from_numpy(R.gram64(y, reg))
    y64 = np.abs(y.astype(np.float64))
    bound = 2 * n * U32 * torch.from_numpy(y64.T @ y64) + U32 * g64.abs()
    print(f'als gram {n}x{f}: worst error / bound {float(((got.double() - g64).abs() / bound).max()):.3f}')
    _assert_bound(got, g64, bound, f'gram {n}x{f}')
    _assert_bits(run_gram(y, reg, ldy=f, ldg=f), got, 'a second run on contiguous operands')
    assert torch.equal(got, got.t()), 'G is not symmetric bit for bit'
    assert torch.equal(S().ops.als_gram(torch.from_numpy(y).to(DEV), reg).cpu(), got)


# ---- sbr_als_solve_rows_f32 through the raw entry point ---------------------------------------------------------------------------------
#        users, items, f, density, alpha, reg, weighted
CASES = {'130x90/f7': (130, 90, 7, 0.1, 40, 0.01, False), '130x90/f64': (130, 90, 64, 0.1, 40, 0.01, False),
         '200x700/f128': (200, 700, 128, 0.3, 40, 0.01, False), '160x700/f100': (160, 700, 100, 0.3, 2, 0.1, False),
         '150x140/f128': (150, 140, 128, 0.2, 0.5, 0.1, False), '60x50/f128': (60, 50, 128, 0.2, 40, 1.0, False),
         '130x90/f1': (130, 90, 1, 0.1, 40, 0.01, False), '130x90/f65': (130, 90, 65, 0.1, 40, 0.01, False),
         '130x90/f64/weighted': (130, 90, 64, 0.1, 40, 0.01, True)}


@functools.lru_cache(maxsize=None)
def sweep_case(name, side):
    """(x, y, g32, yardstick rows, yardstick backward error): the user sweep solves the rows of world(users, items) against item factors,
    the item sweep the rows of world(items, users), the matrix in the place of X^T, against user factors"""
    users, items, f, density, alpha, reg, weighted = CASES[name]
    n, m = (users, items) if side == 'user' else (items, users)
    x = R.world(n, m, density, seed=users + items + f + (side == 'item'), weighted=weighted)
    y = R.uniform_factors(m, f, seed=7 * f + (side == 'item'))
    g = R.gram32(y, reg)
    ref = R.half_sweep32(x, y, alpha, g)
    return x, y, g, ref, R.backward_error(x, y, g, alpha, ref)


def run_solve(x, y, g, alpha, ranges=None, ldx=None, ldy=None, info_out=None):
    """raw sbr_als_solve_rows_f32 over the row ranges (default: all rows in one call) into a NaN-filled guarded buffer -> the [n, f] view
    on the host; nothing outside the ranges' rows x [0, f) was written"""
    n, f = x.shape[0], y.shape[1]
    ranges = ranges or [(0, n)]
    ops = [_i64(x.indptr), _i32(x.indices), None if bool((x.data == 1).all()) else torch.from_numpy(x.data.astype(np.float32)).to(DEV)]
    yb = _Buf(y.shape[0], f, ld=ldy or f, off=0 if ldy is None else 1, data=torch.from_numpy(y))
    out = _Buf(n, f, ld=ldx or f, off=0 if ldx is None else 1)
    gd = torch.from_numpy(g).to(DEV).contiguous()
    info = torch.zeros(1, device=DEV, dtype=torch.int32)
    written = torch.zeros(n, dtype=torch.bool)
    for r0, r1 in ranges:
        call('sbr_als_solve_rows_f32', *[_p(o) for o in ops], r0, r1, yb.ptr, y.shape[0], yb.ld, f, _p(gd), float(alpha), out.ptr, out.ld,
             _p(info), _L().stream())
        written[r0:r1] = True
    if info_out is not None:
        info_out.append(int(info.item()))
    else:
        assert int(info.item()) == 0, f'info = {int(info.item())}'
    return out.check_untouched(written, what=f'solve rows {ranges}').contiguous()


@pytest.mark.parametrize('side', ['user', 'item'])
@pytest.mark.parametrize('name', list(CASES))
def test_half_sweep(name, side):
    x, y, g, ref, be_ref = sweep_case(name, side)
    alpha = CASES[name][4]
    n, f = x.shape[0], y.shape[1]
    got = run_solve(x, y, g, alpha, ldx=f + 3, ldy=f + 5)                           # (c) the guard bands are checked inside
    be = R.backward_error(x, y, g, alpha, got.numpy())
    fwd = np.abs(got.double().numpy() - R.half_sweep64(x, y, alpha, 0., g=g)).max() / np.abs(ref).max()
    print(f'als solve {name} {side}: backward error kernel {be:.3e} yardstick {be_ref:.3e} ratio {be / be_ref:.3f}; forward {fwd:.3e}')
    assert be <= R.BACKWARD_FACTOR * be_ref                                         # (a)
    assert bool((got[1] == 0).all()) and not bool(torch.signbit(got[1]).any())      # (b) the empty row: +0.0
    assert bool(torch.isfinite(got).all())
    # (d) the bits do not depend on the row range, on the strides or on the run
    split = run_solve(x, y, g, alpha, ranges=[(0, 37), (37, 38), (38, n)])
    _assert_bits(split, got, 'three ranges against one')
    prev = S().ops.set_deterministic(True)                                          # (e) valid in deterministic mode, and counted as such
    try:
        before = S().ops.nondeterministic_launches()
        _assert_bits(run_solve(x, y, g, alpha), got, 'a second run, in deterministic mode')
        assert S().ops.nondeterministic_launches() == before
    finally:
        S().ops.set_deterministic(prev)
    part = run_solve(x, y, g, alpha, ranges=[(2, 5)], ldx=f + 1)                    # rows outside [2, 5) keep their NaN
    assert torch.equal(part[2:5], got[2:5]) and bool(torch.isnan(part[:2]).all()) and bool(torch.isnan(part[5:]).all())


def test_half_sweep_in_deterministic_mode_and_through_ops():
    Sm = S()
    x, y, g, _, _ = sweep_case('130x90/f64/weighted', 'user')
    got = run_solve(x, y, g, 40)
    feats = __import__('importlib').import_module(Sm.ops.__name__.rsplit('.', 1)[0] + '.features')
    csr = feats.DeviceCSR(x).to(DEV)
    assert csr.data is not None
    yd, gd = torch.from_numpy(y).to(DEV), torch.from_numpy(g).to(DEV)
    prev = Sm.ops.set_deterministic(True)
    try:
        before = Sm.ops.nondeterministic_launches()
        det = run_solve(x, y, g, 40)                                                # (e)
        via_ops = Sm.ops.als_solve_rows(csr, yd, gd, 40)
        g_ops = Sm.ops.als_gram(yd, 0.01)
        torch.cuda.synchronize()
        assert Sm.ops.nondeterministic_launches() == before
    finally:
        Sm.ops.set_deterministic(prev)
    _assert_bits(det, got, 'deterministic mode')
    _assert_bits(via_ops.cpu(), got, 'ops.als_solve_rows')
    assert tuple(g_ops.shape) == (64, 64)
    big = torch.full((x.shape[0], 70), 7.25, device=DEV)
    assert Sm.ops.als_solve_rows(csr, yd, gd, 40, out=big[:, :64], rows=(10, 20)).data_ptr() == big.data_ptr()
    assert torch.equal(big[10:20, :64].cpu(), got[10:20]) and bool((big[:10] == 7.25).all()) and bool((big[20:] == 7.25).all())
    assert bool((big[:, 64:] == 7.25).all())
    fresh = Sm.ops.als_solve_rows(csr, yd, gd, 40, rows=(10, 20))
    assert torch.equal(fresh[10:20].cpu(), got[10:20]) and not bool(fresh[:10].any()) and not bool(fresh[20:].any())


# ---- error returns ----------------------------------------------------------------------------------------------------------------------
def test_a_bad_pivot_is_an_error_return():
    Sm = S()
    x, y, _, _, _ = sweep_case('130x90/f7', 'user')
    info = []
    # returns normally. Row 2 holds one entry: A[0][0] = -1 + 39 y^2 < 0 whatever y in (-0.5 / 7, 0.5 / 7) is
    run_solve(x, y, -np.eye(7, dtype=np.float32), 40, ranges=[(2, 60)], info_out=info)
    assert info == [1 + 2]
    feats = __import__('importlib').import_module(Sm.ops.__name__.rsplit('.', 1)[0] + '.features')
    csr = feats.DeviceCSR(x).to(DEV)
    with pytest.raises(Sm.SibrarHipError, match=r'row 0 .*regularization.*f \* 2\^-24'):
        Sm.ops.als_solve_rows(csr, torch.from_numpy(y).to(DEV), -torch.eye(7, device=DEV), 40)
    ok = Sm.ops.als_solve_rows(csr, torch.from_numpy(y).to(DEV), torch.eye(7, device=DEV), 40)   # and the next call starts clean
    assert bool(torch.isfinite(ok).all())


def test_refusals_name_the_entry_point():
    Sm = S()
    x, y, g, _, _ = sweep_case('130x90/f7', 'user')
    n = x.shape[0]
    ops = [_i64(x.indptr), _i32(x.indices)]
    yd, gd, out = torch.from_numpy(y).to(DEV), torch.from_numpy(g).to(DEV), torch.zeros(n, 7, device=DEV)
    info = torch.zeros(1, device=DEV, dtype=torch.int32)

    def solve(f=7, alpha=40., ldx=7, ldy=7, r0=0, r1=n):
        call('sbr_als_solve_rows_f32', _p(ops[0]), _p(ops[1]), None, r0, r1, _p(yd), y.shape[0], ldy, f, _p(gd), alpha, _p(out), ldx, _p(info),
             _L().stream())
    for kw, word in (({'f': 129, 'ldx': 129, 'ldy': 129}, 'f=129'), ({'alpha': 0.}, 'alpha'), ({'ldx': 6}, 'leading dimension'),
                     ({'ldy': 6}, 'leading dimension'), ({'r0': 5, 'r1': 4}, 'row range')):
        with pytest.raises(Sm.SibrarHipError, match=f'sbr_als_solve_rows_f32.*{word}'):
            solve(**kw)
    assert not bool(out.any()) and int(info.item()) == 0
    with pytest.raises(Sm.SibrarHipError, match='sbr_als_gram_f32.*reg'):
        Sm.ops.als_gram(yd, 0.)
    with pytest.raises(Sm.SibrarHipError, match='sbr_als_gram_f32.*f=129'):
        Sm.ops.als_gram(torch.zeros(4, 129, device=DEV), 0.1)
    with pytest.raises(ValueError, match='rows'):
        Sm.ops.als_solve_rows(SimpleNamespace(shape=(n, 91), indptr=ops[0], indices=ops[1], data=None), yd, gd, 40)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
MODELS = {'200x700/f128': (200, 700, 128, 0.3, 40, 0.01), '130x90/f64': (130, 90, 64, 0.1, 40, 0.01)}
SEED = 11


@functools.lru_cache(maxsize=None)
def model_case(name):
    users, items, f, density, alpha, reg = MODELS[name]
    x = R.world(users, items, density, seed=users + f)
    m = S().AlternatingLeastSquare(alpha, f, reg, 3, random_state=SEED).fit(x)
    u0, i0 = m.initial_factors(users, items)
    u64, i64 = R.fit64(x, u0, i0, alpha, reg, 3)
    u32, i32 = R.fit32(x, u0, i0, alpha, reg, 3)
    return x, m, u64 @ i64.T, u32.astype(np.float64) @ i32.astype(np.float64).T


@pytest.mark.parametrize('name', list(MODELS))
def test_fit_meets_the_float64_fit(name):
    Sm = S()
    users, items, f, density, alpha, reg = MODELS[name]
    x, m, s64, s32 = model_case(name)
    assert m.users_factors.dtype == torch.float32 and tuple(m.users_factors.shape) == (users, f) and tuple(m.items_factors.shape) == (items, f)
    assert m.users_factors.device.type == 'cuda'
    got = m.users_factors.cpu().double().numpy() @ m.items_factors.cpu().double().numpy().T
    dev, dev_ref = np.abs(got - s64).max() / np.abs(s64).max(), np.abs(s32 - s64).max() / np.abs(s64).max()
    print(f'ALS fit {name}: score deviation kernel {dev:.3e} yardstick {dev_ref:.3e} ratio {dev / dev_ref:.3f}')
    assert dev <= R.SCORE_FACTOR * dev_ref
    # the same fit, one half-sweep at a time: the float64 loss never goes up, and the bits are the fit's
    feats = __import__('importlib').import_module(Sm.ops.__name__.rsplit('.', 1)[0] + '.features')
    csr, csr_t = feats.DeviceCSR(x).to(DEV), feats.DeviceCSR(R.canonical(x.T)).to(DEV)
    u, i = (torch.from_numpy(a).to(DEV) for a in m.initial_factors(users, items))
    trace = [R.loss64(x, u.cpu().numpy(), i.cpu().numpy(), alpha, reg)]
    for _ in range(3):
        u = Sm.ops.als_solve_rows(csr, i, Sm.ops.als_gram(i, reg), alpha)
        trace.append(R.loss64(x, u.cpu().numpy(), i.cpu().numpy(), alpha, reg))
        i = Sm.ops.als_solve_rows(csr_t, u, Sm.ops.als_gram(u, reg), alpha)
        trace.append(R.loss64(x, u.cpu().numpy(), i.cpu().numpy(), alpha, reg))
    print(f'ALS fit {name}: loss {[f"{v:.6e}" for v in trace]}')
    assert all(b <= a for a, b in zip(trace, trace[1:])), trace
    assert torch.equal(u, m.users_factors) and torch.equal(i, m.items_factors)
    again = Sm.AlternatingLeastSquare(alpha, f, reg, 3, random_state=SEED).fit(x)
    assert torch.equal(again.users_factors, m.users_factors) and torch.equal(again.items_factors, m.items_factors)


@pytest.mark.parametrize('name', list(MODELS))
def test_predict_and_combine(name):
    users, items, f = MODELS[name][:3]
    _, m, _, _ = model_case(name)
    rng = np.random.default_rng(3)
    u = torch.from_numpy(rng.integers(0, users, size=33))
    i = torch.from_numpy(rng.integers(0, items, size=(33, 9)))
    u_repr, i_repr = m.get_user_representations(u), m.get_item_representations(torch.arange(items))
    assert torch.is_tensor(u_repr) and torch.is_tensor(i_repr) and tuple(u_repr.shape) == (33, f) and tuple(i_repr.shape) == (items, f)
    full = m.combine_user_item_representations(u_repr, i_repr)
    pred = m.predict(u, i)
    assert pred.dtype == torch.float32 and tuple(pred.shape) == (33, 9)
    assert torch.equal(pred, torch.gather(full, 1, i.to(DEV)))
    u64, i64 = u_repr.cpu().double(), i_repr.cpu().double()
    bound = 2 * f * U32 * (u64.abs() @ i64.abs().t())
    print(f'ALS combine {name}: worst error / bound {float(((full.cpu().double() - u64 @ i64.t()).abs() / bound).max()):.3f}')
    _assert_bound(full.cpu(), u64 @ i64.t(), bound, 'combine')


def test_persistence_needs_no_attach(tmp_path):
    Sm = S()
    _, m, _, _ = model_case('130x90/f64')
    u, i = torch.arange(0, 130, 7), torch.arange(90).expand(19, 90)
    m.save_model_to_path(str(tmp_path))
    back = Sm.AlternatingLeastSquare(40, 64, 0.01, 3)
    back.load_model_from_path(str(tmp_path))
    assert torch.equal(back.predict(u, i), m.predict(u, i))


# ---- evaluation ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted():
    """a planted rank-8 0/1 world, 300 users x 200 items, one interaction per user held out -> (train matrix, evaluation view)"""
    rng = np.random.default_rng(8)
    score = rng.normal(size=(300, 8)) @ rng.normal(size=(200, 8)).T
    d = (score > np.quantile(score, 0.85)).astype(np.float64)
    lab = np.zeros_like(d)
    for u in range(300):
        held = np.flatnonzero(d[u])
        if len(held) < 2:
            held = np.argsort(-score[u])[:2]
            d[u, held] = 1
        pick = rng.choice(held)
        d[u, pick], lab[u, pick] = 0, 1
    train, lab = R.canonical(sp.csr_matrix(d)), R.canonical(sp.csr_matrix(lab))
    view = SimpleNamespace(n_users=300, n_items=200, items_in_split=np.arange(200), users_in_split=np.arange(300), n_items_in_split=200,
                           n_users_in_split=300, user_sampling_matrix=lab, exclude_data=train.astype(bool))
    return train, view


def _evaluate(m, scorer):
    Sm = S()
    _, view = planted()
    loader = type('L', (), {'dataset': view, 'batch_size': 64})()
    ev = Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=(5, 10), metrics=('ndcg', 'recall')), dataset=view)
    lib = _L()
    lib.CALL_LOG = []
    try:
        res = Sm.evaluate_recommender_algorithm(m, loader, ev, DEV, scorer=scorer)
    finally:
        log, lib.CALL_LOG = lib.CALL_LOG, None
    return res, [name for name, _ in log]


def test_evaluation_on_the_fp32_and_the_fused_route():
    Sm = S()
    train, _ = planted()
    m = Sm.AlternatingLeastSquare(40, 64, 0.01, 3, random_state=SEED).fit(train)
    start = Sm.AlternatingLeastSquare(40, 64, 0.01, 0, random_state=SEED).fit(train)          # the random initial factors
    plain, log = _evaluate(m, 'fp32')
    assert not any(n.startswith('sbr_score_topk') for n in log)
    fused, log_fused = _evaluate(m, 'fp32_fused')
    assert 'sbr_score_topk_f32s' in log_fused
    base, _ = _evaluate(start, 'fp32')
    print(f'ALS evaluation: ndcg@10 fp32 {plain["ndcg@10"]:.4f} fp32_fused {fused["ndcg@10"]:.4f} initial factors {base["ndcg@10"]:.4f}')
    for res in (plain, fused):
        assert all(np.isfinite(v) for v in res.values() if isinstance(v, (float, np.floating))) and 0. <= res['ndcg@10'] <= 1.
        assert {'ndcg@5', 'ndcg@10', 'recall@5', 'recall@10'} <= set(res)
    assert plain['ndcg@10'] > base['ndcg@10']
