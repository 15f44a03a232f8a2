"""No GPU: the references of tests/rankpos_ref.py for the rank-position metrics (dcg, ap, rr) on hand-worked lists whose answers are
written out here, the fp32 restatement inside the derived bounds of the float64 definitions on the very inputs the GPU module feeds the
kernel, the branches those inputs must reach, and ``paired_significance`` (eval/stat_tests.py:15-38) against a t-test worked by hand."""
import math

import numpy as np
import pytest

import evalk_ref as E
import rankpos_ref as R


def _csr(*rows):
    return R.csr_of([np.asarray(r, dtype=np.int32) for r in rows])


def _both(top, u, csr, ks):
    top = np.asarray(top, dtype=np.int32)
    return R.pos_metrics_ref64(top, u, csr, ks), R.pos_metrics_f32(top, u, csr, ks)


def test_hand_worked_lists():
    # hits at ranks 0 and 2, n_pos = 3
    csr = _csr([10, 20, 30])
    top = [[10, 99, 30, 98, 97]]
    r64, r32 = _both(top, None, csr, [1, 2, 3, 5])
    assert r64[2].reshape(-1).tolist() == [1.0, 1.0, 1.0, 1.0]
    assert r64[0].reshape(-1).tolist() == [1.0, 1.0, 1.0 + 1.0 / 2.0, 1.0 + 1.0 / 2.0]                    # log2(2) = 1, log2(4) = 2
    assert r64[1].reshape(-1).tolist() == [1.0 / 1.0, 1.0 / 2.0, (1.0 / 1.0 + 2.0 / 3.0) / 3.0, (1.0 / 1.0 + 2.0 / 3.0) / 3.0]
    f = np.float32
    assert r32[0].reshape(-1).tolist() == [1.0, 1.0, 1.5, 1.5] and r32[2].reshape(-1).tolist() == [1.0] * 4
    assert r32[1].reshape(-1).tolist() == [f(1), f(0.5), (f(1) + f(2) / f(3)) / f(3), (f(1) + f(2) / f(3)) / f(3)]
    # the first hit at rank 3: rr = 1/4 from k = 4 on, dcg = 1 / log2(5), ap = (1/4) / min(k, n_pos)
    top = [[99, 98, 97, 20, 96]]
    r64, r32 = _both(top, None, csr, [3, 4, 5])
    assert r64[2].reshape(-1).tolist() == [0.0, 0.25, 0.25]
    assert r64[0].reshape(-1).tolist() == [0.0, 1.0 / math.log2(5.0), 1.0 / math.log2(5.0)]
    assert r64[1].reshape(-1).tolist() == [0.0, 0.25 / 3.0, 0.25 / 3.0]
    assert r32[2].reshape(-1).tolist() == [0.0, 0.25, 0.25] and r32[1].reshape(-1).tolist() == [0.0, f(0.25) / f(3), f(0.25) / f(3)]
    # a perfect list: ap = 1 at every cut-off, also past n_pos
    r64, r32 = _both([[30, 10, 20, 99, 98]], None, csr, [1, 2, 3, 4, 5])
    assert r64[1].reshape(-1).tolist() == [1.0, 1.0, 1.0, 1.0, 1.0] and r32[1].reshape(-1).tolist() == [1.0, 1.0, 1.0, 1.0, 1.0]


def test_no_positives_gives_zero_everywhere():
    csr = _csr([], [5])
    r64, r32 = _both([[5, 6, 7], [1, 2, 3]], None, csr, [1, 3])
    assert not r64[:, :, 0].any() and not r32[:, :, 0].any()                  # n_pos = 0: item 5 is user 1's label, not user 0's
    assert not r64[:, :, 1].any() and not r32[:, :, 1].any()                  # positives, no hit
    assert not np.isnan(r32).any()


def test_ap_divides_by_n_pos_once_k_exceeds_it():
    csr = _csr([1, 2])
    r64, r32 = _both([[1, 9, 2, 8, 7, 6]], None, csr, [1, 2, 3, 6])
    assert r64[1].reshape(-1).tolist() == [1.0 / 1.0, 1.0 / 2.0, (1.0 + 2.0 / 3.0) / 2.0, (1.0 + 2.0 / 3.0) / 2.0]      # min(k, 2)
    f = np.float32
    assert r32[1].reshape(-1).tolist() == [f(1), f(0.5), (f(1) + f(2) / f(3)) / f(2), (f(1) + f(2) / f(3)) / f(2)]


def test_minus_one_is_never_a_hit():
    csr = _csr([0, 3])                                                         # item 0 is a label: a -1 must not be read as item 0
    r64, r32 = _both([[-1, -1, 3, -1]], None, csr, [2, 4])
    assert r64[2].reshape(-1).tolist() == [0.0, 1.0 / 3.0] and r64[0].reshape(-1).tolist() == [0.0, 0.5]
    assert r64[1].reshape(-1).tolist() == [0.0, (1.0 / 3.0) / 2.0]
    assert r32[2].reshape(-1).tolist() == [0.0, np.float32(1) / np.float32(3)]


def test_u_idx_picks_the_label_row():
    csr = _csr([7], [8])
    r64, _ = _both([[7, 8], [7, 8]], np.array([1, 1]), csr, [2])
    assert r64[2].reshape(-1).tolist() == [0.5, 0.5]


def test_given_discounts_replace_log2():
    csr = _csr([1, 2, 3])
    disc = np.float32([0.75, 0.5, 0.125, 0.0625])
    got = R.pos_metrics_f32(np.int32([[1, 9, 2, 3]]), None, csr, [4], disc=disc)
    assert got[0, 0, 0] == (np.float32(0.75) + np.float32(0.125)) + np.float32(0.0625)


@pytest.mark.parametrize('kmax', R.POS_KMAX)
def test_kernel_inputs_restatement_inside_the_bounds_and_every_branch_met(kmax):
    met = set()
    for Bu in R.POS_BU:
        for permuted in (False, True):
            top, u, csr = R.pos_world(Bu, kmax, permuted)
            assert top.shape == (Bu, kmax) and top.dtype == np.int32 and top.max() < R.N_ITEMS
            assert all(len(set(row[row >= 0].tolist())) == (row >= 0).sum() for row in top), 'a list repeats an item'
            met |= R.branches_met(top, u, csr)
            hit, npos = E.hits_and_npos(top, u, csr)
            for ks in R.pos_ks_sets(kmax):
                assert all(1 <= k <= kmax for k in ks) and sorted(set(ks)) == list(ks) and len(ks) <= 8
                what = f'Bu {Bu} kmax {kmax} permuted {permuted} ks {ks}'
                r64, r32 = R.pos_metrics_ref64(top, u, csr, ks), R.pos_metrics_f32(top, u, csr, ks)
                assert r32.dtype == np.float32 and not np.isnan(r32).any(), what
                assert (np.abs(r32[0] - r64[0]) <= R.dcg_bound(top, u, csr, ks)).all(), f'{what}: dcg'
                b = R.ap_rr_bounds(top, u, csr, ks)
                assert (np.abs(r32[1] - r64[1]) <= b[0]).all() and (np.abs(r32[2] - r64[2]) <= b[1]).all(), f'{what}: ap / rr'
                assert (r64[1:] >= 0).all() and (r64[1:] <= 1).all() and (r32[1:] >= 0).all() and (r32[1:] <= 1).all(), f'{what}: range'
                # dcg / idcg, clamped, is the ndcg of the existing float64 reference (two float64 sums of at most kmax terms each)
                nd = E.metrics_ref64(top, u, csr, ks).numpy()[0]
                idcg = R.idcg_ref64(npos, ks)
                mine = np.where(npos > 0, np.minimum(r64[0] / np.where(npos > 0, idcg, 1.0), 1.0), 0.0)
                assert (np.abs(mine - nd) <= 4 * kmax * 2.0 ** -53).all(), f'{what}: dcg / idcg is not ndcg'
    assert met >= R.branches_expected(kmax), f'kmax {kmax}: the inputs miss {sorted(R.branches_expected(kmax) - met)}'
    sets = R.pos_ks_sets(kmax)
    for k in (1, 64, 65, kmax):
        assert k > kmax or any(k in ks for ks in sets), f'kmax {kmax}: no cut-off {k}'


def test_single_hit_lists_isolate_one_term():
    top, u, csr = R.single_hit_world(300)
    r64 = R.pos_metrics_ref64(top, u, csr, [300])
    assert np.array_equal(r64[0, 0], 1.0 / np.log2(np.arange(300) + 2.0)) and np.array_equal(r64[2, 0], 1.0 / (np.arange(300) + 1.0))
    disc = np.arange(300, dtype=np.float32) + 3
    assert np.array_equal(R.pos_metrics_f32(top, u, csr, [300], disc=disc)[0, 0], disc)


def test_evaluator_world_is_what_the_gpu_test_assumes():
    full, items, calls, csr, cat = R.evaluator_world()
    assert full.shape == (260, 450) and len(items) == 400 and len(R.EVAL_KS) == 11 and max(R.EVAL_KS) > 64
    assert set(cat.tolist()) == {0, 1}
    lab = full.tocsr()[:, items]
    lab.sort_indices()
    assert np.array_equal(lab.indptr, csr[0]) and np.array_equal(lab.indices, csr[1])
    assert sum(len(ids) for ids, _ in calls) == 280 and all(top.shape == (len(ids), 70) and top.max() < 400 for ids, top in calls)
    met = set().union(*(R.branches_met(top, ids, csr) for ids, top in calls))
    assert met >= {'hit at rank 0', 'hit at rank 63', 'hit at rank 64', 'hit at the last rank', 'the whole list hits', 'n_pos = 0',
                   'n_pos = 1', 'n_pos > kmax', 'padded with -1', 'no hit with positives'}


# ---- paired_significance ----------------------------------------------------------------------------------------------------------
def _sig():
    import sibrar_amd
    return sibrar_amd.paired_significance


def _p_two_sided_2dof(t):
    """Student's t with 2 degrees of freedom has the closed-form CDF F(t) = 1/2 + t / (2 sqrt(2 + t^2)); two-sided p = 2 (1 - F(|t|))"""
    t = abs(t)
    return 2.0 * (1.0 - (0.5 + t / (2.0 * math.sqrt(2.0 + t * t))))


def test_paired_significance_against_a_t_test_worked_by_hand():
    # differences [1, 2, 3]: mean 2, sample standard deviation 1, t = 2 / (1 / sqrt(3)) = 2 sqrt(3) on 2 degrees of freedom
    base = np.array([0.25, 0.5, 0.125])
    res = _sig()({'a': base + np.array([1.0, 2.0, 3.0]), 'b': base})
    p = _p_two_sided_2dof(2.0 * math.sqrt(3.0))
    assert res['best'] == 'a' and res['threshold'] == 0.05 and set(res['p_values']) == {'b'}
    assert abs(res['p_values']['b'] - p) <= 1e-12 * p, (res['p_values']['b'], p)
    assert res['significant'] == {'b': False} and p > 0.05
    assert _sig()({'a': base + np.array([1.0, 2.0, 3.0]), 'b': base}, threshold=0.1)['significant'] == {'b': True} and p <= 0.1


def test_paired_significance_best_threshold_and_nans():
    rng = np.random.default_rng(4)
    x = rng.random(40)
    res = _sig()({'low': x - 0.5 + rng.normal(0, 0.01, 40), 'best': x + 1.0, 'mid': x + rng.normal(0, 0.01, 40), 'mid2': x + 0.5 + rng.normal(0, 0.01, 40)}, threshold=0.06)
    assert res['best'] == 'best' and set(res['p_values']) == {'low', 'mid', 'mid2'}
    assert res['threshold'] == 0.06 / 3
    assert all(res['significant'][m] == (res['p_values'][m] <= 0.06 / 3) for m in res['p_values'])
    # pairwise omission: a NaN on either side drops the pair and nothing else -> the three-pair case above
    a = np.array([1.25, np.nan, 2.5, 3.125, 7.0])
    b = np.array([0.25, 5.0, 0.5, 0.125, np.nan])
    res = _sig()({'a': a, 'b': b})
    p = _p_two_sided_2dof(2.0 * math.sqrt(3.0))
    assert res['best'] == 'a' and abs(res['p_values']['b'] - p) <= 1e-12 * p


def test_paired_significance_refuses_one_model_and_unequal_lengths():
    with pytest.raises(ValueError, match='at least two'):
        _sig()({'only': np.arange(5.0)})
    with pytest.raises(ValueError, match='same users'):
        _sig()({'a': np.arange(5.0), 'b': np.arange(4.0)})
