"""csrc/svd.hip on the GPU. sbr_sym_eig_f32 against float32 LAPACK (numpy.linalg.eigh) on the same input as the yardstick: every figure
may be 8 x the yardstick's, with an absolute floor of n * 2^-24 only where the yardstick is exactly zero; sbr_gram_f32 and
sbr_csr_times_dense_f32 against float64 within the bound of a sum of that many terms; SVDAlgorithm against the float64 SVD with the
float32 block iteration of tests/svd_ref.py from the same initial block as the yardstick (model <= 10 x yardstick), and through the
hooks and evaluate_recommender_algorithm. Every figure is printed before it is asserted.

numpy's float32 eigh converts to double, calls LAPACK there and rounds the results, so the yardstick's figures are those of a correctly
rounded answer (7e-9 to 7e-8): the kernel meets them because it iterates in double as well (a float32 Jacobi iteration measured 8 to
86 x at n >= 64, and 16.7 x on the rank-deficient matrix at n = 7)."""
import functools
import logging
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import svd_ref as R
from hip_testutil import DEV, GUARD, NAN, S, U32, _Buf, _assert_bits, _assert_bound, _bits, _i32, _i64, _L, _p, call

pytestmark = pytest.mark.gpu


def _feats():
    return __import__('importlib').import_module(S().ops.__name__.rsplit('.', 1)[0] + '.features')


# ---- sbr_sym_eig_f32 --------------------------------------------------------------------------------------------------------------------
def run_eig(a, lda, ldw, info_word=0):
    """raw sbr_sym_eig_f32 inside guarded NaN-filled buffers -> (lam, W, info) on the host"""
    n = a.shape[0]
    ab = _Buf(n, n, ld=lda, off=1, data=torch.from_numpy(a))
    wb = _Buf(n, n, ld=ldw, off=1)
    lb = _Buf(1, n, off=1)
    info = torch.full((1,), info_word, device=DEV, dtype=torch.int32)
    need = int(_L().lib().sbr_sym_eig_f32_workspace(n))
    ws = torch.full((need // 8 + 2 * GUARD,), NAN, device=DEV, dtype=torch.float64)
    call('sbr_sym_eig_f32', ab.ptr, n, ab.ld, wb.ptr, wb.ld, lb.ptr, _p(info), ws[GUARD:].data_ptr(), need, _L().stream())
    assert bool(torch.isnan(ws[:GUARD]).all()) and bool(torch.isnan(ws[GUARD + need // 8:]).all()), 'written outside the workspace'
    assert torch.equal(ab.check_untouched(what='A').contiguous(), torch.from_numpy(a)), 'the input was written'
    return lb.check_untouched(what='lam').contiguous()[0].numpy(), wb.check_untouched(what='W').contiguous().numpy(), int(info.item())


def _against(fig, ref, n, what):
    """fig <= 8 x ref, or <= n * 2^-24 where ref is exactly zero -> the ratio (inf where ref is zero and fig is not)"""
    ratio = fig / ref if ref > 0 else (0.0 if fig == 0 else float('inf'))
    print(f'    {what}: kernel {fig:.3e} LAPACK {ref:.3e} ratio {ratio:.2f}')
    return (fig <= R.EIG_FACTOR * ref) if ref > 0 else (fig <= n * R.EPS), ratio


@pytest.mark.parametrize('n', [1, 2, 3, 7, 64, 65, 127, 128])
def test_sym_eig(n):
    failures = []
    for name, a in R.eig_inputs(n).items():
        print(f'sym_eig n={n} {name}')
        lam, w, info = run_eig(a, lda=n + 3, ldw=n + 5)
        assert info == 0 and np.isfinite(lam).all() and np.isfinite(w).all()
        lam32, w32 = R.eigh32(a)
        (res, orth), (res32, orth32) = R.eig_figures(a, lam, w), R.eig_figures(a, lam32, w32)
        checks = [_against(res, res32, n, 'residual'), _against(orth, orth32, n, 'orthogonality')]
        if name == 'graded':
            l64 = np.linalg.eigvalsh(a.astype(np.float64))[::-1]
            checks.append(_against(float((np.abs(lam - l64) / np.abs(l64)).max()), float((np.abs(lam32 - l64) / np.abs(l64)).max()), n,
                                   'relative eigenvalue error'))
        failures += [f'{name}: ratio {r:.1f}' for ok, r in checks if not ok]
        assert bool((np.diff(lam) <= 0).all()), 'not descending'
        assert bool((w[np.abs(w).argmax(axis=0), np.arange(n)] > 0).all()), 'the sign rule'
        if name.startswith('diagonal'):
            assert np.array_equal(lam, np.sort(np.diag(a))[::-1]) and np.array_equal(np.abs(w).sum(axis=0), np.ones(n, dtype=np.float32))
        lam2, w2, _ = run_eig(a, lda=n, ldw=n)
        assert np.array_equal(lam2.view(np.int32), lam.view(np.int32)) and np.array_equal(w2.view(np.int32), w.view(np.int32)), 'a second run'
        if name == 'gram':
            l_ops, w_ops = S().ops.sym_eig(torch.from_numpy(a).to(DEV))
            assert np.array_equal(l_ops.cpu().numpy(), lam) and np.array_equal(w_ops.cpu().numpy(), w)
    assert not failures, failures


def test_sym_eig_refusals_and_the_error_return():
    Sm = S()
    a = torch.eye(4, device=DEV)
    w, lam, info = torch.full((4, 4), 7.25, device=DEV), torch.full((4,), 7.25, device=DEV), torch.zeros(1, device=DEV, dtype=torch.int32)
    ws = torch.zeros(129 * 130, device=DEV, dtype=torch.float64)
    for n in (0, 129):
        with pytest.raises(Sm.SibrarHipError, match=f'sbr_sym_eig_f32: n={n}'):
            call('sbr_sym_eig_f32', _p(a), n, 200, _p(w), 200, _p(lam), _p(info), _p(ws), 8 * ws.numel(), _L().stream())
    with pytest.raises(Sm.SibrarHipError, match='sbr_sym_eig_f32: workspace of 64 bytes, 128 needed'):
        call('sbr_sym_eig_f32', _p(a), 4, 4, _p(w), 4, _p(lam), _p(info), _p(ws), 64, _L().stream())
    assert bool((w == 7.25).all()) and bool((lam == 7.25).all()) and int(info.item()) == 0          # nothing was launched
    # info is only ever set, never cleared: a word that is set on entry stands for a run that reached the cap
    lam_h, _, word = run_eig(np.eye(4, dtype=np.float32), 4, 4, info_word=31)
    assert word == 31 and np.array_equal(lam_h, np.ones(4, dtype=np.float32))
    with pytest.raises(Sm.SibrarHipError, match=r'sym_eig: .*sweep 30.*info = 31'):
        Sm.ops.sym_eig(a, info=torch.full((1,), 31, device=DEV, dtype=torch.int32))
    lam_ok, w_ok = Sm.ops.sym_eig(a)                                                               # and the next call starts clean
    assert torch.equal(lam_ok, torch.ones(4, device=DEV)) and torch.equal(w_ok, a)
    with pytest.raises(ValueError, match='float32 only'):
        Sm.ops.sym_eig(a.double())
    with pytest.raises(ValueError, match='square'):
        Sm.ops.sym_eig(torch.zeros(3, 4, device=DEV))
    with pytest.raises(ValueError, match='outside'):
        Sm.ops.sym_eig(torch.eye(129, device=DEV))


# ---- sbr_gram_f32 -----------------------------------------------------------------------------------------------------------------------
def run_gram(entry, y, ldy, ldg, *reg):
    n, f = y.shape
    yb = _Buf(n, f, ld=ldy, off=1, data=torch.from_numpy(y))
    g = _Buf(f, f, ld=ldg, off=1)
    need = int(_L().lib().sbr_als_gram_f32_workspace(n, f))
    ws = torch.empty(max(need // 4, 1), device=DEV)
    call(entry, yb.ptr, n, yb.ld, f, *reg, g.ptr, g.ld, _p(ws), need, _L().stream())
    return g.check_untouched(what=f'{entry} {n}x{f}').contiguous()


@pytest.mark.parametrize('n,f', [(1, 1), (130, 7), (700, 65), (3000, 128)])
def test_gram(n, f):
    y = np.random.default_rng(n + f).standard_normal((n, f)).astype(np.float32)
    got = run_gram('sbr_gram_f32', y, f + 3, f + 5)
    y64 = y.astype(np.float64)
    g64, bound = torch.from_numpy(y64.T @ y64), 2 * n * U32 * torch.from_numpy(np.abs(y64).T @ np.abs(y64))
    print(f'gram {n}x{f}: worst error / bound {float(((got.double() - g64).abs() / bound).max()):.3f}')
    _assert_bound(got, g64, bound, f'gram {n}x{f}')
    assert torch.equal(got, got.t()), 'G is not symmetric bit for bit'
    _assert_bits(run_gram('sbr_gram_f32', y, f, f), got, 'a second run on contiguous operands')
    assert torch.equal(S().ops.gram(torch.from_numpy(y).to(DEV)).cpu(), got)
    reg = 0.25
    als = run_gram('sbr_als_gram_f32', y, f, f, reg)
    off = ~torch.eye(f, dtype=torch.bool)
    assert torch.equal(als[off], got[off])
    assert torch.equal(torch.diagonal(als), torch.diagonal(got) + np.float32(reg))                  # reg is added last: one rounding


# ---- sbr_csr_times_dense_f32 ------------------------------------------------------------------------------------------------------------
def product_world(n, m, weighted, seed):
    """a random n x m matrix with row 1 empty, row 2 holding a single entry and row 3 full (small shapes: what there is room for)"""
    rng = np.random.default_rng(seed)
    d = (rng.random((n, m)) < 0.15).astype(np.float64)
    if n > 3:
        d[1], d[2], d[3] = 0, 0, 1
        d[2, m // 2] = 1
    if weighted:
        d *= rng.uniform(-2, 2, size=d.shape)
    return R.canonical(sp.csr_matrix(d))


def run_times(indptr, indices, data, n, D, ranges=None, ldd=None, ldo=None):
    c = D.shape[1]
    db = _Buf(D.shape[0], c, ld=ldd or c, off=0 if ldd is None else 1, data=torch.from_numpy(D))
    out = _Buf(n, c, ld=ldo or c, off=0 if ldo is None else 1)
    written = torch.zeros(n, dtype=torch.bool)
    for r0, r1 in ranges or [(0, n)]:
        call('sbr_csr_times_dense_f32', _p(indptr), _p(indices), _p(data), r0, r1, db.ptr, D.shape[0], db.ld, c, out.ptr, out.ld, _L().stream())
        written[r0:r1] = True
    return out.check_untouched(written, what=f'csr x dense {ranges}').contiguous()


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('n,m,c', [(1, 1, 1), (130, 90, 7), (130, 90, 64), (130, 90, 65), (130, 90, 128), (90, 130, 65)])
def test_csr_times_dense(n, m, c, weighted):
    Sm = S()
    x = product_world(n, m, weighted, seed=n + c)
    D = np.random.default_rng(c).standard_normal((m, c)).astype(np.float32)
    ops = [_i64(x.indptr), _i32(x.indices), torch.from_numpy(x.data.astype(np.float32)).to(DEV) if weighted else None]
    got = run_times(*ops, n, D, ldd=c + 3, ldo=c + 5)
    x64, x32 = np.asarray(x.todense()), np.asarray(x.astype(np.float32).todense(), dtype=np.float64)
    nnz = torch.from_numpy(np.diff(x.indptr).astype(np.float64))[:, None]
    bound = nnz * U32 * torch.from_numpy(np.abs(x32) @ np.abs(D.astype(np.float64)))
    ref = torch.from_numpy(x32 @ D.astype(np.float64))
    print(f'csr x dense {n}x{m} c={c} weighted={weighted}: worst error / bound {float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max()):.3f}')
    _assert_bound(got, ref, bound, 'csr x dense')
    empty = np.flatnonzero(np.diff(x.indptr) == 0)
    assert n == 1 or 1 in empty
    assert not bool(_bits(got[empty]).any()), 'an empty row is not +0.0f bit for bit'
    if n > 3:
        _assert_bits(run_times(*ops, n, D, ranges=[(0, 37), (37, 38), (38, n)]), got, 'three ranges against one')
        part = run_times(*ops, n, D, ranges=[(2, 5)], ldo=c + 1)
        assert torch.equal(part[2:5], got[2:5]) and bool(torch.isnan(part[:2]).all()) and bool(torch.isnan(part[5:]).all())
    prev = Sm.ops.set_deterministic(True)
    try:
        before = Sm.ops.nondeterministic_launches()
        _assert_bits(run_times(*ops, n, D), got, 'a second run, in deterministic mode')
        assert Sm.ops.nondeterministic_launches() == before
    finally:
        Sm.ops.set_deterministic(prev)
    # through ops, and the transposed operand of DeviceCSR.transposed()
    csr = _feats().DeviceCSR(x).to(DEV)
    assert torch.equal(Sm.ops.csr_times_dense(csr, torch.from_numpy(D).to(DEV)).cpu(), got)
    t_indptr, t_indices, t_data = csr.transposed()
    xt = SimpleNamespace(shape=(m, n), indptr=t_indptr, indices=t_indices, data=t_data)
    Dt = np.random.default_rng(c + 1).standard_normal((n, c)).astype(np.float32)
    got_t = Sm.ops.csr_times_dense(xt, torch.from_numpy(Dt).to(DEV)).cpu()
    nnz_t = torch.from_numpy(np.asarray((x64 != 0).sum(axis=0)).reshape(-1).astype(np.float64))[:, None]
    _assert_bound(got_t, torch.from_numpy(x32.T @ Dt.astype(np.float64)), nnz_t * U32 * torch.from_numpy(np.abs(x32.T) @ np.abs(Dt.astype(np.float64))),
                  'the transposed operand')
    big = torch.full((n, c + 6), 7.25, device=DEV)
    if n > 20:
        assert Sm.ops.csr_times_dense(csr, torch.from_numpy(D).to(DEV), out=big[:, :c], rows=(10, 20)).data_ptr() == big.data_ptr()
        assert torch.equal(big[10:20, :c].cpu(), got[10:20]) and bool((big[:10] == 7.25).all()) and bool((big[20:] == 7.25).all())


def test_ops_refuse_wrong_operands():
    Sm = S()
    csr = _feats().DeviceCSR(sp.csr_matrix(np.eye(3))).to(DEV)
    with pytest.raises(ValueError, match='D has 4 rows'):
        Sm.ops.csr_times_dense(csr, torch.zeros(4, 2, device=DEV))
    with pytest.raises(ValueError, match='float32'):
        Sm.ops.csr_times_dense(csr, torch.zeros(3, 2, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match='unit column stride'):
        Sm.ops.csr_times_dense(csr, torch.zeros(2, 3, device=DEV).t())
    with pytest.raises(ValueError, match='outside'):
        Sm.ops.csr_times_dense(csr, torch.zeros(3, 129, device=DEV))
    with pytest.raises(ValueError, match='row range'):
        Sm.ops.csr_times_dense(csr, torch.zeros(3, 2, device=DEV), rows=(2, 5))
    with pytest.raises(ValueError, match='outside'):
        Sm.ops.gram(torch.zeros(3, 129, device=DEV))
    with pytest.raises(ValueError, match='float32'):
        Sm.ops.gram(torch.zeros(3, 4, device=DEV, dtype=torch.float16))


# ---- the model ------------------------------------------------------------------------------------------------------------------------
#        world, factors
MODELS = {'130x90/g5': ('130x90/g5', 5), '300x200/g8': ('300x200/g8', 8), '700x260/g16': ('700x260/g16', 16), '300x200/f1': ('300x200/g8', 1),
          '300x200/f64': ('300x200/g8', 64)}
SEED = 11


@functools.lru_cache(maxsize=None)
def world(name):
    x = R.planted(*R.WORLDS[name])
    u, s, vt = R.svd64(x)
    g = R.WORLDS[name][2]
    assert s[g - 1] >= 1.3 * s[g], 'the planted world lost its spectral gap'
    return x, u, s, vt


@functools.lru_cache(maxsize=None)
def model_case(name):
    wname, f = MODELS[name]
    x = world(wname)[0]
    m = S().SVDAlgorithm(f, random_state=SEED).fit(x)
    b = min(f + m.oversample, *x.shape)
    return x, m, R.fit32(x, m.initial_block(x.shape[1], b), f, m.n_iterations, m.tol)


@pytest.mark.parametrize('name', list(MODELS))
def test_fit_meets_the_float64_svd(name):
    Sm = S()
    wname, f = MODELS[name]
    _, u64, s64, vt64 = world(wname)
    x, m, (u32, v32, s32, it32, hist32) = model_case(name)
    assert m.users_factors.dtype == torch.float32 and tuple(m.users_factors.shape) == (x.shape[0], f)
    assert tuple(m.items_factors.shape) == (x.shape[1], f) and m.users_factors.device.type == 'cuda' and tuple(m.singular_values.shape) == (f,)
    uf, vf, sv = m.users_factors.cpu().double().numpy(), m.items_factors.cpu().double().numpy(), m.singular_values.cpu().double().numpy()
    print(f'SVD fit {name}: {m.n_iterations_run} iterations (fit32 {it32}), residual {m.residual / sv[0]:.3e} s_0 (fit32 {hist32[-1] / s32[0]:.3e}); '
          f'history {[f"{r / sv[0]:.1e}" for r in m.residual_history]}')
    dev_s, ref_s = np.abs(sv - s64[:f]).max() / s64[0], np.abs(s32 - s64[:f]).max() / s64[0]
    print(f'SVD fit {name}: singular values kernel {dev_s:.3e} yardstick {ref_s:.3e} ratio {dev_s / ref_s:.2f}')
    orth, orth_ref = np.abs(vf.T @ vf - np.eye(f)).max(), np.abs(v32.astype(np.float64).T @ v32.astype(np.float64) - np.eye(f)).max()
    print(f'SVD fit {name}: V^T V - I kernel {orth:.3e} yardstick {orth_ref:.3e} ratio {orth / orth_ref:.2f}')
    assert m.residual <= m.tol * sv[0] and m.n_iterations_run < m.n_iterations
    assert dev_s <= R.MODEL_FACTOR * ref_s
    if f != 64:                                                                    # no gap behind 64: the scores are not determined
        p64 = (u64[:, :f] * s64[:f]) @ vt64[:f]
        dev, ref = np.abs(uf @ vf.T - p64).max() / np.abs(p64).max(), np.abs(u32.astype(np.float64) @ v32.astype(np.float64).T - p64).max() / np.abs(p64).max()
        print(f'SVD fit {name}: scores kernel {dev:.3e} yardstick {ref:.3e} ratio {dev / ref:.2f}')
        assert dev <= R.MODEL_FACTOR * ref
        assert orth <= R.MODEL_FACTOR * orth_ref
    assert bool((np.diff(sv) <= 0).all())
    again = Sm.SVDAlgorithm(f, random_state=SEED).fit(x)
    assert torch.equal(again.users_factors, m.users_factors) and torch.equal(again.items_factors, m.items_factors)
    assert torch.equal(again.singular_values, m.singular_values) and again.n_iterations_run == m.n_iterations_run


def test_no_iteration_returns_the_orthonormalised_start():
    x = world('130x90/g5')[0]
    m = S().SVDAlgorithm(5, random_state=SEED, n_iterations=0).fit(x)
    v = m.items_factors.cpu().double().numpy()
    assert m.n_iterations_run == 0 and tuple(v.shape) == (90, 5) and np.abs(v.T @ v - np.eye(5)).max() <= 1e-5
    ref = np.asarray(x.todense()) @ v
    assert np.abs(m.users_factors.cpu().double().numpy() - ref).max() <= 1e-5 * np.abs(ref).max()


def test_the_gapless_world(caplog):
    n_users, n_items, g = R.GAPLESS[:3]
    x = R.planted(*R.GAPLESS)
    s64 = R.svd64(x)[1]
    with caplog.at_level(logging.WARNING):
        m = S().SVDAlgorithm(g, random_state=SEED).fit(x)
    sv = m.singular_values.cpu().double().numpy()
    b = min(g + m.oversample, n_users, n_items)
    assert b == 128
    s32 = R.fit32(x, m.initial_block(n_items, b), g, m.n_iterations, m.tol)[2]
    dev_s, ref_s = np.abs(sv - s64[:g]).max() / s64[0], np.abs(s32 - s64[:g]).max() / s64[0]
    met = m.residual <= m.tol * sv[0]
    print(f'SVD gapless: {m.n_iterations_run} iterations, residual {m.residual / sv[0]:.3e} s_0, tol met: {met}; singular values kernel {dev_s:.3e} '
          f'yardstick {ref_s:.3e} ratio {dev_s / ref_s:.2f}')
    assert dev_s <= R.MODEL_FACTOR * ref_s
    warned = [r for r in caplog.records if 'SVDAlgorithm' in r.getMessage() and 'residual' in r.getMessage()]
    assert bool(warned) == (not met)


def test_a_nan_is_refused_before_any_launch():
    d = np.eye(6)
    d[1, 2] = np.nan
    lib = _L()
    lib.CALL_LOG = []
    try:
        with pytest.raises(ValueError, match='non-finite'):
            S().SVDAlgorithm(2).fit(sp.csr_matrix(d))
    finally:
        log, lib.CALL_LOG = lib.CALL_LOG, None
    assert log == []


# ---- the surface ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted_rank8():
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
    _, view = planted_rank8()
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
    train, _ = planted_rank8()
    m8 = Sm.SVDAlgorithm(8, random_state=SEED).fit(train)
    rng = np.random.default_rng(3)
    u, i = torch.from_numpy(rng.integers(0, 300, size=33)), torch.from_numpy(rng.integers(0, 200, size=(33, 9)))
    full = m8.combine_user_item_representations(m8.get_user_representations(u), m8.get_item_representations(torch.arange(200)))
    pred = m8.predict(u, i)
    assert pred.dtype == torch.float32 and tuple(pred.shape) == (33, 9) and torch.equal(pred, torch.gather(full, 1, i.to(DEV)))
    m8.save_model_to_path(str(tmp_path))
    back = Sm.SVDAlgorithm(8)
    back.load_model_from_path(str(tmp_path))                                       # no attach: the factors are the model
    assert torch.equal(back.predict(u, i), pred)
    plain8, log8 = _evaluate(m8, 'fp32')
    loaded8, _ = _evaluate(back, 'fp32')
    assert not any(n.startswith('sbr_score_topk') for n in log8) and loaded8['ndcg@10'] == plain8['ndcg@10']
    m64 = Sm.SVDAlgorithm(64, random_state=SEED).fit(train)
    start = Sm.SVDAlgorithm(64, random_state=SEED, n_iterations=0).fit(train)       # the orthonormalised random start
    plain, _ = _evaluate(m64, 'fp32')
    fused, log_fused = _evaluate(m64, 'fp32_fused')
    base, _ = _evaluate(start, 'fp32')
    print(f'SVD evaluation: ndcg@10 factors 8 {plain8["ndcg@10"]:.4f}; factors 64 fp32 {plain["ndcg@10"]:.4f} fp32_fused {fused["ndcg@10"]:.4f}; '
          f'random start {base["ndcg@10"]:.4f}')
    assert 'sbr_score_topk_f32s' in log_fused
    assert fused['ndcg@10'] == plain['ndcg@10']
    assert plain8['ndcg@10'] > 2 * base['ndcg@10'] and plain8['ndcg@10'] > 0.1
