"""tests/block_ref.py on CPU arithmetic only: the case lists hold what they promise; the exact inputs meet the 2^24 conditions their bit
comparisons rely on; a numpy float32 restatement of the order that include/sibrar_hip.h states passes every checker at the shapes
tests/test_hip_block_edges.py runs (the condition that makes the bounds legitimate: the stated arithmetic alone passes them); and each
listed wrong restatement is rejected by every checker it can reach: the last row of a slab dropped, the first row of a slab added
twice, columns 0 and 64 exchanged, the row's diagonal in place of the column's, s without the floor, 1 / s applied before the chain.
That is how the GPU tests are known to fail on a subtly wrong kernel; no GPU test tries to make a kernel misbehave. No GPU."""
import numpy as np
import pytest

import block_ref as B


def rejected(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


def test_case_lists():
    for cases, rows, widths in ((B.ROT_CASES, B.ROT_N, B.ROT_B), (B.GRAM_CASES, B.GRAM_N, B.GRAM_F)):
        assert {n for n, _ in cases} == set(rows) and {w for _, w in cases} == set(widths)
        assert all(sum(1 for c in cases if c[1] == w) >= 2 for w in widths) and all(sum(1 for c in cases if c[0] == n) >= 2 for n in rows)
    assert len(B.RES_CASES) == len(B.RES_N) * len(B.RES_F)
    assert {n for n, _ in B.GRAM_FLOAT_CASES} == set(B.GRAM_N)
    for weighted in (False, True):
        indptr, indices, data = B.als_world(weighted)
        nnz = list(np.diff(indptr))
        assert set(nnz) >= {0, 1, 23, 24, 25, 47, 48, 49, B.ALS_NY} and nnz[1] == 0 and (data is not None) == weighted
        for r in range(len(nnz)):
            row = indices[indptr[r]:indptr[r + 1]]
            assert bool((np.diff(row) > 0).all()) and (len(row) == 0 or (row[0] >= 0 and row[-1] < B.ALS_NY))
    assert B.EASE_N_WRAP == 4096 + 1 and B.slabs(513, B.RES_SLAB) == 3 and B.slabs(512, B.GRAM_SLAB) == 1 and B.slabs(1025, B.GRAM_SLAB) == 3


def test_exact_inputs_are_exact():
    for n, b in B.ROT_CASES:
        B.assert_exact_rotate(*B.rotate_exact_inputs(n, b))
    for n, f in B.RES_CASES:
        for kind in ('zero', 'squares'):
            Y, Um, s, expected = B.col_residual_inputs(n, f, kind)
            B.assert_exact_col_residual(Y, Um, s)
            assert np.array_equal(expected, np.rint(expected)) and (kind == 'squares' or not expected.any())
        if n > B.RES_SLAB:                                         # both sides of the first slab boundary carry a one in every column
            Y, Um, s, _ = B.col_residual_inputs(n, f, 'squares')
            d = Y.astype(np.float64) - s.astype(np.float64)[None, :] * Um
            assert bool((d[B.RES_SLAB - 1] == 1).all()) and bool((d[B.RES_SLAB] == 1).all())
    for n, f in B.GRAM_CASES:
        B.assert_exact_gram(B.gram_inputs(n, f, 'int'))


def test_the_floor_branches_are_all_reached():
    for b in B.ROT_B:
        if b < 7:
            continue
        lam = B.rotate_lam(b, 'relative floor', 1).astype(np.float64)
        floor = lam[0] * 2.0 ** -46
        assert floor > 2.0 ** -126 and (lam == 0).any() and (lam < 0).any() and ((lam > 0) & (lam < floor)).any()
        lam = B.rotate_lam(b, 'FLT_MIN floor', 1).astype(np.float64)
        assert 0 < lam[0] * 2.0 ** -46 < 2.0 ** -126 and ((lam > 0) & (lam < 2.0 ** -126)).any() and (lam < 0).any()
        s = B.rotate_s32(B.rotate_lam(b, 'FLT_MIN floor', 1))
        assert (s == np.float32(2.0 ** -63)).any() and s[0] > np.float32(2.0 ** -63)
        assert B.rotate_lam(b, 'lam[0] zero', 1)[0] == 0 and B.rotate_s32(B.rotate_lam(b, 'lam[0] zero', 1))[0] == np.float32(2.0 ** -63)


# ---- the restatements inside the bounds -------------------------------------------------------------------------------------------------
def test_rotate_restatement():
    worst = 0.0
    for n, b in B.ROT_CASES:
        Y, W = B.rotate_exact_inputs(n, b)
        for i, kind in enumerate(B.LAM_KINDS):
            lam = B.rotate_lam(b, kind, seed=n + b + i)
            out, s = B.rotate32(Y, W, lam)
            B.check_rotate_exact(out, s, Y, W, lam)
        B.check_rotate_exact(B.rotate32(Y, W)[0], None, Y, W, None)
        Y, W, lam = B.rotate_float_inputs(n, b)
        out, s = B.rotate32(Y, W, lam)
        worst = max(worst, B.check_rotate_float(out, s, Y, W, lam))
    print(f'rotate restatement: worst error / bound {worst:.3f}')


def test_col_residual_restatement():
    worst = {'float': 0.0, 'cancel': 0.0}
    for n, f in B.RES_CASES:
        for kind in ('zero', 'squares'):
            Y, Um, s, expected = B.col_residual_inputs(n, f, kind)
            B.check_col_residual_exact(B.col_residual32(Y, Um, s), Y, Um, s, expected)
        for kind in worst:
            Y, Um, s, _ = B.col_residual_inputs(n, f, kind)
            worst[kind] = max(worst[kind], B.check_col_residual_float(B.col_residual32(Y, Um, s), Y, Um, s))
    print(f'col residual restatement: worst error / bound {worst}')


def test_ease_restatement():
    for n in B.EASE_N:
        P = B.ease_inputs(n)
        B.check_ease(B.ease_weights32(P), P)
        assert n == 1 or not np.array_equal(P, P.T)
        d = np.diagonal(P)
        assert bool((d != 0).all()) and (n == 1 or ((d > 0).any() and (d < 0).any()))


def test_gram_restatement():
    worst = 0.0
    for n, f in B.GRAM_CASES:
        Y = B.gram_inputs(n, f, 'int')
        B.check_gram_exact(B.gram32(Y), Y)
        B.check_gram_exact(B.gram32(Y, B.GRAM_REG), Y, B.GRAM_REG)
    for n, f in B.GRAM_FLOAT_CASES:
        Y = B.gram_inputs(n, f, 'float')
        worst = max(worst, B.check_gram_float(B.gram32(Y), Y), B.check_gram_float(B.gram32(Y, B.GRAM_REG), Y, B.GRAM_REG))
    print(f'gram restatement: worst error / bound {worst:.3f}')


@pytest.mark.parametrize('weighted', [False, True])
def test_als_restatement(weighted):
    for f in B.ALS_F:
        ratio = B.check_als(B.als_restated32(f, weighted), f, weighted)
        print(f'als restatement f={f} weighted={weighted}: backward error / ({B.BACKWARD_FACTOR} x yardstick) {ratio:.3f}')


def test_tri_and_cholesky_restatements():
    for r in B.TRI_R:
        b, T = B.tri_inputs(r)
        for upper in (0, 1):
            for unit in (0, 1):
                tt = np.triu(T) if upper else np.tril(T)
                ratio = B.check_tri(B.tri_solve32(b, tt, upper, unit), b, T, upper, unit)
                print(f'tri restatement r={r} upper={upper} unit={unit}: worst residual / bound {ratio:.3f}')
    for n in B.CHOL_N:
        K = B.chol_input(n)
        print(f'cholesky restatement n={n}: worst residual / bound {B.check_chol(B.chol32(K), K):.3f}')


# ---- the wrong restatements outside them ------------------------------------------------------------------------------------------------
def test_rotate_checkers_reject_the_mutants():
    n, b = next(c for c in B.ROT_CASES if c[1] == 65)
    Y, W = B.rotate_exact_inputs(n, b)
    for i, kind in enumerate(B.LAM_KINDS):
        lam = B.rotate_lam(b, kind, seed=i)
        for mutant in ('no_tiny_floor', 'scale_before_chain', 'swap_0_64'):
            out, s = B.rotate32(Y, W, lam, mutant)
            rejected(B.check_rotate_exact, out, s, Y, W, lam)
    rejected(B.check_rotate_exact, B.rotate32(Y, W, None, 'swap_0_64')[0], None, Y, W, None)
    Y, W, lam = B.rotate_float_inputs(n, b)
    out, s = B.rotate32(Y, W, lam, 'swap_0_64')
    rejected(B.check_rotate_float, out, s, Y, W, lam)
    # b = 1: the floor is all there is to get wrong
    Y, W = B.rotate_exact_inputs(1, 1)
    lam = B.rotate_lam(1, 'lam[0] zero', seed=0)
    out, s = B.rotate32(Y, W, lam, 'no_tiny_floor')
    rejected(B.check_rotate_exact, out, s, Y, W, lam)


@pytest.mark.parametrize('n,f', [(257, 65), (513, 128)])
def test_col_residual_checkers_reject_the_mutants(n, f):
    for mutant in ('drop_last_of_slab', 'double_first_of_slab', 'swap_0_64'):
        Y, Um, s, expected = B.col_residual_inputs(n, f, 'squares')
        rejected(B.check_col_residual_exact, B.col_residual32(Y, Um, s, mutant), Y, Um, s, expected)
        for kind in ('float', 'cancel'):
            Y, Um, s, _ = B.col_residual_inputs(n, f, kind)
            rejected(B.check_col_residual_float, B.col_residual32(Y, Um, s, mutant), Y, Um, s)


def test_ease_checker_rejects_the_rows_diagonal():
    for n in (2, 300):
        P = B.ease_inputs(n)
        rejected(B.check_ease, B.ease_weights32(P, 'row_diagonal'), P)
    sym = (B.ease_inputs(300) + B.ease_inputs(300).T).astype(np.float32)               # what the model feeds: the mix-up is invisible there
    assert np.array_equal(B.ease_weights32(sym, 'row_diagonal'), B.ease_weights32(sym).T)


@pytest.mark.parametrize('n,f', [(513, 65), (1025, 127), (1024, 128)])
def test_gram_checkers_reject_the_mutants(n, f):
    for mutant in ('drop_last_of_slab', 'double_first_of_slab', 'swap_0_64'):
        Y = B.gram_inputs(n, f, 'int')
        rejected(B.check_gram_exact, B.gram32(Y, 0.0, mutant), Y)
        rejected(B.check_gram_exact, B.gram32(Y, B.GRAM_REG, mutant), Y, B.GRAM_REG)
        Y = B.gram_inputs(n, f, 'float')
        rejected(B.check_gram_float, B.gram32(Y, 0.0, mutant), Y)


def test_row_solver_checkers_reject_exchanged_columns():
    for f in (65, 128):
        rejected(B.check_als, B.als_restated32(f, True, 'swap_0_64'), f, True)
    wrong = B.als_restated32(65, False).copy()
    wrong[1, 3] = -0.0
    rejected(B.check_als, wrong, 65, False)                                              # the empty row must be +0.0 in every bit
    for r in (65, 127):
        b, T = B.tri_inputs(r)
        rejected(B.check_tri, B.tri_solve32(b, np.tril(T), 0, 0, 'swap_0_64'), b, T, 0, 0)
    K = B.chol_input(127)
    R = B.chol32(K)
    R[:, [0, 64]] = R[:, [64, 0]]
    rejected(B.check_chol, R, K)
