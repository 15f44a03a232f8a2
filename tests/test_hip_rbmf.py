"""csrc/rbmf.hip on the GPU against tests/rbmf_ref.py. The float64 restatement is the oracle; decisions (pivot rows, swaps) are compared
only on inputs on which every runner-up / winner ratio of the oracle is <= 1 - 1e-4, and that is asserted. Every figure is printed
before it is asserted.

Bounds. u = 2^-24, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.):
  LU chain     the computed factors satisfy L U = A + dA with |dA| <= gamma_r |L| |U| (Thm 9.3, any order of the r terms, a division per
               multiplier; a fused multiply-add rounds less, not more). It is evaluated in float64 from the kernel's own L (all rows) and
               Utop against the input: the elementwise agreement with float64 that holds for every conditioning of the leading blocks
               (a forward bound on L itself needs their condition numbers). Ltop is L[idx] bit for bit.
  tri solve    the computed row satisfies x (T + dT) = b with |dT| <= gamma_r |T| (Thm 8.5): |x T - b| <= gamma_r |x| |T| in float64.
  Cholesky     R R^T = K + dK with |dK| <= gamma_(n+1) |R| |R^T| (Thm 10.3).
  certificate  max |U inv(U[idx])| in float64 from the returned idx alone is <= tol + slack, slack = max(10 x the excess over tol of the
               numpy float32 restatement on the same input, r * 2^-23).
  model        the error of X against the float64 closed form from the model's own representatives is <= 10 x the error of the numpy
               float32 restatement of the same formula, written as the reference writes it (an explicit inverse and a product)."""
import functools
import importlib
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import rbmf_ref as R
from hip_testutil import DEV, S, _Buf, _bits, _L, _p, call

pytestmark = pytest.mark.gpu

RS = (1, 2, 63, 64, 65, 100, 128)
SLAB = 160
SEED = 11


def sizes(r):
    return sorted({n for n in (r, r + 1, SLAB - 1, SLAB + 1, 3 * SLAB + 7) if n >= r})


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


# ---- the LU chain ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', RS)
def test_lu_chain(r):
    ops = S().ops
    for n in sizes(r):
        u, idx64, L64, ltop64, utop64, ratio = R.lu_input(n, r)
        assert ratio <= R.RATIO_MAX
        buf = _Buf(n, r, ld=r + 3, off=1, data=torch.from_numpy(u))
        idx, ltop, utop = ops.maxvol_lu(buf.t, SLAB, want_upper=True)
        L = buf.check_untouched(what=f'LU {n}x{r}').contiguous().double().numpy()   # what lies between the view's rows keeps its bits
        idx, ltop, utop = idx.cpu().numpy(), ltop.cpu().numpy(), utop.cpu().double().numpy()
        assert np.array_equal(idx, idx64), f'pivot order at n={n}'
        resid, bound = np.abs(L @ utop - u.astype(np.float64)), R.gamma(r) * (np.abs(L) @ np.abs(utop))
        fwd = np.abs(L - L64).max()
        print(f'LU r={r} n={n}: ratio {ratio:.5f}, worst residual / bound {float((resid / np.maximum(bound, 1e-300)).max()):.3f}, max |L - L64| {fwd:.2e}')
        assert bool((resid <= bound).all())
        assert np.array_equal(ltop, L[idx].astype(np.float32)) and np.array_equal(np.diag(ltop), np.ones(r, dtype=np.float32))
        assert not np.triu(ltop, 1).any() and not np.tril(utop, -1).any() and np.abs(L).max() <= 1.0
        for slab in (0, 64):                                                    # another slab size: the same bits
            again = dev(u)
            idx2, ltop2, _ = ops.maxvol_lu(again, slab)
            assert np.array_equal(idx2.cpu().numpy(), idx) and torch.equal(_bits(again.cpu()), _bits(torch.from_numpy(L.astype(np.float32))))
            assert np.array_equal(ltop2.cpu().numpy(), ltop)


def test_lu_duplicated_rows_and_a_rank_deficient_block():
    Sm = S()
    u = R.tall(161, 8, 5)
    u[40, 0] = 2                                                                 # the largest element of column 0, and the row's copy
    u[100] = u[40]                                                               # further down: a tie at step 0, an exact zero row afterwards
    idx, _, _ = Sm.ops.maxvol_lu(dev(u), SLAB)
    idx = idx.cpu().numpy()
    assert idx[0] == 40 and 100 not in idx, idx
    assert np.array_equal(idx, R.lu_pivots(u)[0])
    z = R.tall(161, 8, 6)
    z[:, 5] = 0                                                                  # an exact zero pivot at step 5
    with pytest.raises(Sm.SibrarHipError, match=r'maxvol_lu: the pivot of step 5 .*rank below 8.*fewer representatives'):
        Sm.ops.maxvol_lu(dev(z), SLAB)
    d = R.tall(161, 64, 7)
    d[:, 40] = d[:, 3]                                                           # column 40 drowns in rounding once column 3 is eliminated
    with pytest.raises(Sm.SibrarHipError, match=r'maxvol_lu: the pivot of step 40 '):
        Sm.ops.maxvol_lu(dev(d), SLAB)
    with pytest.raises(Sm.SibrarHipError, match='rank below'):
        Sm.ops.maxvol(dev(z))
    idx_ok, _, _ = Sm.ops.maxvol_lu(dev(R.tall(161, 8, 6)), SLAB)                 # and the next call starts clean
    assert len(set(idx_ok.cpu().tolist())) == 8


# ---- sbr_tri_solve_rows_f32 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', RS)
def test_tri_solve_rows(r):
    ops = S().ops
    rng = np.random.default_rng(40 + r)
    n = SLAB + 1
    b = rng.standard_normal((n, r)).astype(np.float32)
    full = (rng.standard_normal((r, r)) / max(np.sqrt(r), 1)).astype(np.float32)
    full[np.arange(r), np.arange(r)] = rng.uniform(1, 2, size=r).astype(np.float32) * rng.choice([-1, 1], size=r)
    for upper in (False, True):
        for unit in (False, True):
            t64 = (np.triu(full) if upper else np.tril(full)).astype(np.float64)
            if unit:
                t64[np.arange(r), np.arange(r)] = 1
            tb = _Buf(r, r, ld=r + 2, off=1, data=torch.from_numpy(full))         # the other triangle and the unit diagonal are not read
            xin = _Buf(n, r, ld=r + 5, off=1, data=torch.from_numpy(b))
            xout = _Buf(n, r, ld=r + 1, off=3)
            ops.tri_solve_rows(xin.t, tb.t, upper=upper, unit=unit, out=xout.t)
            x = xout.check_untouched(what='out').contiguous()
            assert torch.equal(xin.check_untouched(what='in').contiguous(), torch.from_numpy(b))
            x64 = x.double().numpy()
            resid, bound = np.abs(x64 @ t64 - b), R.gamma(r) * (np.abs(x64) @ np.abs(t64))
            print(f'tri solve r={r} upper={upper} unit={unit}: worst residual / bound {float((resid / np.maximum(bound, 1e-300)).max()):.3f}')
            assert bool((resid <= bound).all())
            ops.tri_solve_rows(xin.t, tb.t, upper=upper, unit=unit, out=xin.t)     # in place: the same bits
            assert torch.equal(_bits(xin.check_untouched(what='in place').contiguous()), _bits(x))
    # exact on operands with power-of-two entries: pairs (2k, 2k + 1) are coupled, so every value is a small dyadic number
    t = np.diag(2.0 ** rng.integers(-3, 4, size=r))
    for k in range(0, r - 1, 2):
        t[k + 1, k] = 2.0 ** rng.integers(-2, 3)
    ints = rng.integers(-8, 9, size=(n, r)).astype(np.float64)
    for upper, tm in ((False, t), (True, t.T.copy())):
        got = ops.tri_solve_rows(dev(ints), dev(tm), upper=upper).cpu().double().numpy()
        assert np.array_equal(got, np.linalg.solve(tm.T, ints.T).T), f'upper={upper}'
        unit_t = tm.copy()
        unit_t[np.arange(r), np.arange(r)] = 1
        got = ops.tri_solve_rows(dev(ints), dev(tm), upper=upper, unit=True).cpu().double().numpy()
        assert np.array_equal(got, np.linalg.solve(unit_t.T, ints.T).T), f'upper={upper} unit'


@pytest.mark.parametrize('n', [1, 2, 65, 128])
def test_cholesky(n):
    Sm = S()
    c = (np.random.default_rng(n).random((n, 3 * n + 5)) < 0.3).astype(np.float32)
    k = (c @ c.T + np.float32(1e-2) * np.eye(n, dtype=np.float32)).astype(np.float32)
    kb = _Buf(n, n, ld=n + 3, off=1, data=torch.from_numpy(np.tril(k)))             # the lower triangle is read
    rr = Sm.ops.cholesky(kb.t).cpu().double().numpy()
    resid, bound = np.abs(rr @ rr.T - k), R.gamma(n + 1) * (np.abs(rr) @ np.abs(rr.T))
    print(f'cholesky n={n}: worst residual / bound {float((resid / bound).max()):.3f}')
    assert bool((resid <= bound).all()) and not np.triu(rr, 1).any() and bool((np.diag(rr) > 0).all())
    if n >= 2:
        bad = k.copy()
        bad[1, 1] = bad[1, 0] = bad[0, 1] = bad[0, 0]                             # a singular leading 2 x 2 block
        bad[1, 1] -= 1
        with pytest.raises(Sm.SibrarHipError, match='cholesky: .*pivot 1 '):
            Sm.ops.cholesky(dev(bad))


# ---- the swap chain -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', RS)
def test_swap_chain_from_a_poor_start(r):
    ops = S().ops
    for n in sizes(r):
        u, i64, s64, i32, s32, ratio = R.poor_start_input(n, r)
        assert ratio <= R.RATIO_MAX
        ud = dev(u)
        idx, swaps = ops.maxvol(ud, R.TOL, 4 * 128, SLAB, start=np.arange(r))
        idx = idx.cpu().numpy()
        cert, slack = R.certificate(u, idx), R.slack(u, i32, r)
        print(f'swap chain r={r} n={n}: {swaps} swaps (float64 {s64}, float32 {s32}), ratio {ratio:.5f}, certificate {cert:.7f}, float32 '
              f'restatement {R.certificate(u, i32):.7f}, slack {slack:.2e}')
        assert idx.dtype == np.int64 and set(idx) == set(i64) and swaps == s64
        assert cert <= R.TOL + slack
        assert torch.equal(ud.cpu(), torch.from_numpy(u)), 'U was written'
        for slab in (0, 64):                                                    # two more slab sizes, and so a second run: the same decisions
            idx2, swaps2 = ops.maxvol(ud, R.TOL, 4 * 128, slab, start=np.arange(r))
            assert np.array_equal(idx2.cpu().numpy(), idx) and swaps2 == swaps
        idx0, swaps0 = ops.maxvol(ud, R.TOL, 0, SLAB, start=np.arange(r))
        assert swaps0 == 0 and np.array_equal(idx0.cpu().numpy(), np.arange(r))


@pytest.mark.parametrize('r,n', [(2, 161), (64, 487), (128, 487)])
def test_maxvol_from_the_lu_start_and_the_idle_launches(r, n):
    ops = S().ops
    u = R.lu_input(n, r)[0]
    ud = dev(u)
    lu_idx = ops.maxvol_lu(ud.clone(), SLAB)[0].cpu().numpy()
    idx0, swaps0 = ops.maxvol(ud, R.TOL, 0, SLAB)
    assert swaps0 == 0 and np.array_equal(idx0.cpu().numpy(), lu_idx) and np.array_equal(lu_idx, R.lu_pivots(u)[0])      # max_iters = 0: the LU start
    i64, s64, ratio = R.maxvol(u)
    i32 = R.maxvol(u, dtype=np.float32)[0]
    idx, swaps = ops.maxvol(ud, R.TOL, R.MAX_ITERS, SLAB)
    cert = R.certificate(u, idx.cpu().numpy())
    print(f'maxvol r={r} n={n}: {swaps} swaps (float64 {s64}), ratio {ratio:.5f}, certificate {cert:.7f}')
    assert cert <= R.TOL + R.slack(u, i32, r)
    if ratio <= R.RATIO_MAX:
        assert set(idx.cpu().tolist()) == set(i64) and swaps == s64
    # a chain by hand: once it has converged, further launches change no byte of B, of idx or of the counter
    B = ud.clone()
    idx_d, ltop, _ = ops.maxvol_lu(B, SLAB)
    ops.tri_solve_rows(B, ltop, unit=True, out=B)
    need = int(_L().lib().sbr_maxvol_f32_workspace(n, SLAB))
    ws = torch.zeros(need // 4, device=DEV, dtype=torch.int32)
    counter = torch.zeros(1, device=DEV, dtype=torch.int32)
    step = 0
    while True:
        before = int(counter.item())
        for _ in range(8):
            call('sbr_maxvol_swap_step_f32', _p(B), n, r, r, R.TOL, step, _p(idx_d), _p(counter), _p(ws), need, SLAB, _L().stream())
            step += 1
        if int(counter.item()) - before < 8:
            break
        assert step < 8 * 64
    snap = (B.clone(), idx_d.clone(), counter.clone())
    for _ in range(3):
        call('sbr_maxvol_swap_step_f32', _p(B), n, r, r, R.TOL, step, _p(idx_d), _p(counter), _p(ws), need, SLAB, _L().stream())
        step += 1
    assert torch.equal(_bits(B), _bits(snap[0])) and torch.equal(idx_d, snap[1]) and torch.equal(counter, snap[2])
    if ratio <= R.RATIO_MAX:
        assert set(idx_d.cpu().tolist()) == set(i64) and int(counter.item()) == s64


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
def _svd_module():
    return importlib.import_module(S().ops.__name__.rsplit('.', 1)[0] + '.svd')


@functools.lru_cache(maxsize=None)
def model_case(name):
    nu, ni, g, p_in, p_out, seed, r = R.WORLDS[name]
    x = R.planted(nu, ni, g, p_in, p_out, seed)
    m = S().RBMF(r, 1e-2, random_state=SEED, n_iterations=30).fit(x)
    b = min(r + m.oversample, nu, ni)
    U = _svd_module().block_iteration(R.canonical(x), m.initial_block(ni, b), r, m.n_iterations, m.svd_tol, DEV)[0]
    return x, m, np.ascontiguousarray(U[:, :r].cpu().numpy())


@pytest.mark.parametrize('name', list(R.WORLDS))
def test_fit_meets_the_restatement(name):
    Sm = S()
    x, m, u = model_case(name)
    r = R.WORLDS[name][6]
    i64, s64, ratio = R.maxvol(u)
    i32 = R.maxvol(u, dtype=np.float32)[0]
    reps = m.representatives.cpu().numpy()
    cert = R.certificate(u, reps)
    print(f'RBMF {name}: {m.n_swaps} swaps (float64 {s64}), worst decision ratio {ratio:.5f}, certificate {cert:.7f}')
    assert ratio <= R.RATIO_MAX
    assert m.representatives.dtype == torch.int64 and set(reps) == set(i64) and m.n_swaps == s64 and s64 >= 1
    assert cert <= R.TOL + R.slack(u, i32, r)
    x64, c64 = R.ridge(x, reps, 1e-2)
    x32, _ = R.ridge(x, reps, 1e-2, np.float32, literal=True)
    lu32 = np.abs(R.ridge(x, reps, 1e-2, np.float32)[0] - x64).max() / np.abs(x64).max()
    X, C = m.X.cpu().double().numpy(), m.C.cpu().double().numpy()
    assert m.X is m.users_factors and m.C is m.items_factors and X.shape == (x.shape[0], r) and C.shape == (x.shape[1], r)
    assert np.array_equal(C, c64)                                                # the representatives' rows, 0 / 1
    err, ref = np.abs(X - x64).max() / np.abs(x64).max(), np.abs(x32 - x64).max() / np.abs(x64).max()
    print(f'RBMF {name}: X kernel {err:.3e} float32 restatement {ref:.3e} ratio {err / ref:.2f} (a float32 LU solve: {lu32:.3e})')
    assert err <= R.MODEL_FACTOR * ref
    # the same bits again, also in deterministic mode, and no launch that deterministic mode would have to refuse
    Sm.ops.nondeterministic_launches(reset=True)
    prev = Sm.ops.set_deterministic(True)
    try:
        again = Sm.RBMF(r, 1e-2, random_state=SEED, n_iterations=30).fit(x)
    finally:
        Sm.ops.set_deterministic(prev)
    assert Sm.ops.nondeterministic_launches() == 0
    assert torch.equal(_bits(again.X), _bits(m.X)) and torch.equal(again.C, m.C) and torch.equal(again.representatives, m.representatives)
    assert again.n_swaps == m.n_swaps


@functools.lru_cache(maxsize=None)
def planted_rank8():
    """a planted rank-8 0/1 world, 300 users x 200 items, one interaction per user held out -> (train matrix, evaluation view, labels)"""
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
    train, labels = R.canonical(sp.csr_matrix(d)), R.canonical(sp.csr_matrix(lab))
    view = SimpleNamespace(n_users=300, n_items=200, items_in_split=np.arange(200), users_in_split=np.arange(300), n_items_in_split=200,
                           n_users_in_split=300, user_sampling_matrix=labels, exclude_data=train.astype(bool))
    return train, view, lab


def _evaluate(m, scorer):
    Sm = S()
    view = planted_rank8()[1]
    loader = type('L', (), {'dataset': view, 'batch_size': 64})()
    ev = Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=(5, 10), metrics=('ndcg', 'recall')), dataset=view)
    lib = _L()
    lib.CALL_LOG = []
    try:
        res = Sm.evaluate_recommender_algorithm(m, loader, ev, DEV, scorer=scorer)
    finally:
        log, lib.CALL_LOG = lib.CALL_LOG, None
    return res, [name for name, _ in log]


def test_predict_persistence_and_evaluation(tmp_path):
    Sm = S()
    train, _, lab = planted_rank8()
    m = Sm.RBMF(64, 1e-2, random_state=SEED, n_iterations=30).fit(train)
    rng = np.random.default_rng(3)
    u, i = torch.from_numpy(rng.integers(0, 300, size=33)), torch.from_numpy(rng.integers(0, 200, size=(33, 9)))
    full = m.combine_user_item_representations(m.get_user_representations(u), m.get_item_representations(torch.arange(200)))
    pred = m.predict(u, i)
    assert pred.dtype == torch.float32 and tuple(pred.shape) == (33, 9) and torch.equal(pred, torch.gather(full, 1, i.to(DEV)))
    m.save_model_to_path(str(tmp_path))
    with np.load(tmp_path / 'model.npz', allow_pickle=False) as f:
        assert set(f.files) == {'X', 'C', 'name'}
    back = Sm.RBMF(64)
    back.load_model_from_path(str(tmp_path))                                       # no attach: the factors are the model
    assert torch.equal(back.predict(u, i), pred)
    results = {}
    for scorer, entry in (('fp32', None), ('fp32_fused', 'sbr_score_topk_f32s'), ('fp16_fused', 'sbr_score_topk_f16')):
        results[scorer], log = _evaluate(m, scorer)
        assert (entry in log) if entry else not any(n.startswith('sbr_score_topk') for n in log), (scorer, sorted(set(log)))
        assert {'ndcg@5', 'ndcg@10', 'recall@5', 'recall@10'} <= set(results[scorer])
    loaded, _ = _evaluate(back, 'fp32')
    assert loaded['ndcg@10'] == results['fp32']['ndcg@10']
    # the fp32 route against X C^T in float64: the rank of the held-out item among the items not excluded; a user whose label lies
    # within 1e-5 of the largest score of another candidate may move a rank, and each such user may move a metric by 1 / n_users
    s64 = m.X.cpu().double().numpy() @ m.C.cpu().double().numpy().T
    s64[np.asarray(train.todense()) > 0] = -np.inf
    label = lab.argmax(axis=1)
    own = s64[np.arange(300), label]
    rank = (s64 > own[:, None]).sum(axis=1)
    gap = np.abs(np.where(np.isfinite(s64), s64, np.inf) - own[:, None])
    gap[np.arange(300), label] = np.inf
    near = int((gap.min(axis=1) <= 1e-5 * np.abs(s64[np.isfinite(s64)]).max()).sum())
    for k in (5, 10):
        ndcg, recall = float(np.where(rank < k, 1 / np.log2(rank + 2), 0).mean()), float((rank < k).mean())
        print(f'RBMF evaluation @{k}: fp32 ndcg {results["fp32"][f"ndcg@{k}"]:.6f} recall {results["fp32"][f"recall@{k}"]:.6f}; float64 ndcg {ndcg:.6f} '
              f'recall {recall:.6f}; {near} users with a near-tie; fused {results["fp32_fused"][f"ndcg@{k}"]:.6f} fp16 {results["fp16_fused"][f"ndcg@{k}"]:.6f}')
        assert abs(results['fp32'][f'ndcg@{k}'] - ndcg) <= near / 300 + 1e-6 and abs(results['fp32'][f'recall@{k}'] - recall) <= near / 300 + 1e-6
    assert results['fp32_fused']['ndcg@10'] == results['fp32']['ndcg@10']
    assert results['fp32']['ndcg@10'] > 0.1
