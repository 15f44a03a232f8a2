"""The references of tests/evalk_ref.py on CPU arithmetic only: the ordering reference against torch.topk and a stable torch.sort, the
merge reference against parallel.merge_topk, the float64 metrics against oracle/eval_ref.py; the fp32 restatement of
rank_metrics_kernel inside the derived NDCG bound — and bit-exact in recall and precision — on every input set that
tests/test_hip_evalk.py generates (the condition that makes the bound legitimate: the reference arithmetic alone passes it); and each
listed wrong kernel — a mutation of the restatement or of the ordering reference — rejected by the very checks the GPU module applies
(evalk_ref.check_metrics, evalk_ref.same_lists). No GPU."""
import numpy as np
import pytest
import torch

import evalk_ref as E
import test_hip_evalk as G

ALL_I = G.TOPK_I_RADIX + G.TOPK_I_SAMPLED + G.TOPK_I_LONG
SMALL_I = [I for I in ALL_I if I <= 8453]


# ---- ordering -----------------------------------------------------------------------------------------------------------------
def test_topk_ref_equals_torch_topk_on_finite_rows_without_ties():
    g = torch.Generator().manual_seed(3)
    for I, k in ((1, 1), (7, 7), (300, 33), (5000, 256)):
        sc = torch.randn(6, I, generator=g)
        assert all(len(set(r.tolist())) == I for r in sc), 'the test wants rows without ties'
        tv, ti = torch.topk(sc, k, sorted=True)
        val, idx = E.topk_ref(sc, k)
        assert torch.equal(val, tv) and torch.equal(idx.long(), ti)


@pytest.mark.parametrize('I', ALL_I)
def test_topk_ref_equals_the_stable_descending_sort_on_the_gpu_inputs(I):
    """NaN of both signs first and in index order, -0 == +0, ties by index: torch.sort(descending=True, stable=True) agrees"""
    for group in range(len(G.ROW_GROUPS)):
        sc = G.topk_rows_input(I, group)
        k = min(256, I)
        sv, si = torch.sort(sc, dim=1, descending=True, stable=True)
        val, idx = E.topk_ref(sc, k)
        assert torch.equal(idx.long(), si[:, :k]), f'I {I} group {group}'
        assert E.same_values(val, sv[:, :k])
        assert torch.equal(torch.gather(sc, 1, idx.long()).view(torch.int32), val.view(torch.int32))      # the row's own elements


def test_the_topk_inputs_hold_what_the_gpu_module_promises():
    assert set(G.ROW_GROUPS[0]) | set(G.ROW_GROUPS[1]) == set(G.ROW_KINDS) and all(len(g) == 8 for g in G.ROW_GROUPS)
    assert [G.topk_ks(I) for I in (1, 2, 255, 256, 257)] == [[1], [1, 2], [1, 2, 31, 32, 33, 255], [1, 2, 31, 32, 33, 255, 256]] + [[1, 2, 31, 32, 33, 255, 256]]
    assert [I % 256 for I in (8207, 8453)] == [15, 5] and all(I % 4 for I in (8193, 8207, 8453, 65535))
    for I in (8192, 65536):
        rows = {kind: G.topk_row(kind, I, 1) for kind in G.ROW_KINDS}
        x = rows['max_overflows_the_candidates']
        assert int((x == x.max()).sum()) > 2048 and len(np.unique(x)) > 1000
        z = rows['signed_zeros']
        sign = np.signbit(z[z == 0])
        assert sign[0] and sign.any() and (~sign).any() and int((z == 0).sum()) > 256
        n = rows['nans_scattered']
        nan_at = np.flatnonzero(np.isnan(n))
        bits = n.view(np.uint32)[nan_at]
        assert bits[0] == E.NAN_NEG and set(bits.tolist()) == {E.NAN_NEG, E.NAN_POS} and 256 < len(nan_at) < I // 8
        assert np.isnan(rows['all_nan']).all() and len(set(rows['all_nan'].view(np.uint32).tolist())) == 2
        d = rows['denormals']
        assert (np.abs(d) < 2.0 ** -126).all() and (d != 0).all() and (d < 0).any() and (d > 0).any()


@pytest.mark.parametrize('mutant', E.MUTANTS_ORDER)
def test_wrong_orderings_are_rejected(mutant):
    """ties to the higher index; a NaN with the sign bit set ranked last (what the raw bit key did); every +0 ahead of every -0 (the raw
    bit key again): same_lists, the GPU module's comparison, sees each on the GPU module's rows — and on the kind built for it"""
    target = {'ties_to_the_higher_index': 'heavy_ties', 'negative_nan_last': 'nans_scattered', 'plus_zero_ahead_of_minus_zero': 'signed_zeros'}[mutant]
    seen = set()
    for I in SMALL_I:
        for group, kinds in enumerate(G.ROW_GROUPS):
            sc = G.topk_rows_input(I, group)
            for k in G.topk_ks(I):
                want, got = E.topk_ref(sc, k), E.topk_ref(sc, k, mutant)
                for r, kind in enumerate(kinds):
                    if not E.same_lists((got[0][r:r + 1], got[1][r:r + 1]), (want[0][r:r + 1], want[1][r:r + 1])):
                        seen.add((kind, I, k))
    kinds_seen = {s[0] for s in seen}
    print(f'{mutant}: rejected on {len(seen)} (kind, I, k) cases, kinds {sorted(kinds_seen)}')
    assert target in kinds_seen, f'{mutant}: no GPU input sees it'
    assert {(target, I) for I in SMALL_I if I >= 255} <= {(s[0], s[1]) for s in seen}, f'{mutant}: not seen at every I >= 255'


# ---- mask -----------------------------------------------------------------------------------------------------------------------
def test_mask_ref_by_hand_and_the_mask_inputs():
    csr = (np.array([0, 2, 2, 3]), np.array([0, 4, 2]))
    sc = torch.zeros(2, 5)
    out = E.mask_ref(sc, np.array([2, 0]), csr)
    assert torch.isinf(out).tolist() == [[False, False, True, False, False], [True, False, False, False, True]]
    out = E.mask_ref(sc[:, :2], np.array([2, 0]), csr, item_offset=3)
    assert torch.isinf(out).tolist() == [[False, False], [False, True]]
    indptr, indices = G.mask_world()
    n = np.diff(indptr)
    assert n.max() > 128 and ((n > 64) & (n <= 128)).any() and (n == 0).any() and indices.min() == 0 and indices.max() == G.MASK_I - 1
    for off, w in G.MASK_WINDOWS[:2]:                            # the long rows are cut at both ends of these windows
        long_row = indices[indptr[3]:indptr[4]]
        assert (long_row < off).any() or off == 0
        assert (long_row >= off + w).any() and ((long_row >= off) & (long_row < off + w)).any()
    for Bu in G.MASK_BU:
        _, u = G.mask_case(Bu, True)
        assert u[0] == 3 and (Bu < 3 or u[2] == u[0])


# ---- merge ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('W,Bu,k', [(1, 5, 3), (2, 300, 20), (8, 1000, 20), (8, 77, 32), (4, 50, 1)])
def test_merge_ref_equals_the_host_merge(W, Bu, k):
    """on the inputs of test_hip_kernels.test_merge_topk_kernel_equals_the_host_merge (restated: that module is GPU-only)"""
    import sibrar_amd
    g = torch.Generator().manual_seed(W * 100 + k)
    vals = (torch.randint(0, 40, (W, Bu, k), generator=g).float() / 8).sort(dim=2, descending=True).values
    idxs = torch.stack([torch.stack([torch.randperm(1000, generator=g)[:k] + 1000 * w for _ in range(Bu)]) for w in range(W)]).int()
    n_valid = torch.randint(0, k + 1, (W, Bu), generator=g)
    empty = torch.arange(k)[None, None, :] >= n_valid[..., None]
    idxs[empty] = -1
    vals[empty] = -float('inf')
    rv, ri = sibrar_amd.parallel.merge_topk(torch.cat(list(vals), dim=1), torch.cat(list(idxs), dim=1), k)
    mv, mi = E.merge_ref(vals, idxs, k)
    assert torch.equal(mi, ri.int()) and torch.equal(mv, rv)


def test_merge_ref_by_hand_and_the_merge_inputs():
    inf = float('inf')
    vals = torch.tensor([[[2.0, -inf, -inf]], [[2.0, 0.0, -inf]], [[-0.0, -inf, -inf]]])
    idxs = torch.tensor([[[7, 9, -1]], [[3, 50, -1]], [[40, -1, -1]]], dtype=torch.int32)
    mv, mi = E.merge_ref(vals, idxs, 3)
    assert mi.tolist() == [[3, 7, 40]] and mv.tolist() == [[2.0, 2.0, 0.0]]
    mv, mi = E.merge_ref(vals, idxs, 9)
    assert mi.tolist() == [[3, 7, 40, 50, 9, -1, -1, -1, -1]]          # the real -inf entry (item 9) ahead of the empty slots
    assert mv[0, 4:].tolist() == [-inf] * 5
    assert {W * k for W, k in G.MERGE_SHAPES} >= {64, 65, 255, 256}
    vals, idxs = G.merge_case(8, 257, 32)
    v, i = vals.numpy(), idxs.numpy()
    assert ((i >= 0).sum(axis=2) == 0).any() and ((i >= 0).sum(axis=(0, 2)) == 0).sum() >= 257 // 7
    assert (np.isinf(v) & (i >= 0)).any() and np.isnan(v).any() and (np.signbit(v) & (v == 0)).any() and ((v == 0) & ~np.signbit(v)).any()
    bits = v.view(np.uint32)
    assert (bits[0][np.isnan(v[0])] == E.NAN_NEG).all() and (bits[1][np.isnan(v[1])] == E.NAN_POS).all()


# ---- metrics: float64 against the oracle ------------------------------------------------------------------------------------------
def test_metrics_ref64_equals_the_oracle_on_dense_labels(monkeypatch):
    """oracle/eval_ref.py holds the definitions (eval/metrics.py:4-105) but evaluates its discounts with ``.float()``; here its own code
    runs with that cast widened to float64, so that the two agree to 1e-12. Lists without -1 (the oracle indexes with them)."""
    from oracle import eval_ref
    monkeypatch.setattr(torch.Tensor, 'float', lambda self: self.double())
    n = 0
    for what, top, u, csr, ks in G.metrics_inputs():
        if (top < 0).any():
            top = torch.where(top < 0, torch.full_like(top, G.METRIC_I), top)           # an item nobody likes
        hit, npos = E.hits_and_npos(top, u, csr)
        rows = np.arange(top.shape[0]) if u is None else u
        y = np.zeros((top.shape[0], G.METRIC_I + 1))
        for b, r in enumerate(rows):
            y[b, csr[1][csr[0][r]:csr[0][r + 1]]] = 1.0
        y = torch.from_numpy(y)
        ref = E.metrics_ref64(top, u, csr, ks)
        for q, k in enumerate(ks):
            ii = top[:, :k].long()
            for j, fn in enumerate((eval_ref.ndcg_at_k, eval_ref.recall_at_k, eval_ref.precision_at_k)):
                want = fn(y, ii)
                assert want.dtype == torch.float64
                assert float((ref[j, q] - want).abs().max()) <= 1e-12, f'{what} @{k} metric {j}'
                n += 1
    assert n > 500


# ---- metrics: the fp32 restatement inside the bound, the mutants outside ----------------------------------------------------------
def test_the_metric_inputs_are_not_vacuous():
    """at least a third of the (user, cut-off) pairs have 0 < hits < k, at most a tenth of the users have no positive; and the inputs
    hold what the GPU module lists"""
    pairs = partial = users = empty = 0
    seen_npos, tails, first_last, perfect, over_one = set(), 0, set(), 0, 0
    for what, top, u, csr, ks in G.metrics_inputs():
        hit, npos = E.hits_and_npos(top, u, csr)
        kmax = top.shape[1]
        for k in ks:
            h = hit[:, :k].sum(axis=1)
            pairs += len(h)
            partial += int(((h > 0) & (h < k)).sum())
        users += len(npos)
        empty += int((npos == 0).sum())
        seen_npos |= {('0' if n == 0 else '1' if n == 1 else 'kmax-1' if n == kmax - 1 else 'kmax' if n == kmax else 'kmax+5' if n == kmax + 5 else 'other')
                      for n in npos.tolist()}
        tails += int((top.numpy() < 0).any(axis=1).sum())
        first_last |= set(csr[1][(csr[1] == 0) | (csr[1] == G.METRIC_I - 1)].tolist())
        perfect += int(E.perfect_pairs(top, u, csr, ks).sum())
        over_one += int((E.metrics_f32(top, u, csr, ks, 'no_clamp')[0] > 1).sum())
    print(f'(user, cut-off) pairs {pairs}, with 0 < hits < k {partial} ({partial / pairs:.3f}); users {users}, without positives {empty} '
          f'({empty / users:.3f}); lists with a -1 tail {tails}; perfect pairs {perfect}; pairs above 1 before the clamp {over_one}')
    assert 3 * partial >= pairs and 10 * empty <= users
    assert seen_npos >= {'0', '1', 'kmax-1', 'kmax', 'kmax+5'} and tails > 100 and first_last == {0, G.METRIC_I - 1}
    assert perfect > 100 and over_one > 10
    assert {len(ks) for kmax in G.METRIC_KMAX for ks in G.metric_ks_sets(kmax)} >= {1, 8}
    assert all(any(max(ks) < kmax for ks in G.metric_ks_sets(kmax)) for kmax in (20, 256))


def test_fp32_restatement_stays_inside_the_bound_and_is_exact_in_recall_and_precision():
    worst = 0.0
    for what, top, u, csr, ks in G.metrics_inputs():
        worst = max(worst, E.check_metrics(E.metrics_f32(top, u, csr, ks), top, u, csr, ks, what))
    ds, calls, csr = G.evaluator_world()
    for ids, top in calls:
        worst = max(worst, E.check_metrics(E.metrics_f32(top, ids, csr, G.EVAL_KS), top, ids, csr, G.EVAL_KS, 'evaluator world'))
    print(f'fp32 restatement: worst ndcg err / bound {worst:.4f}')
    assert worst < 1.0


@pytest.mark.parametrize('mutant', E.MUTANTS_METRICS)
def test_wrong_metric_kernels_are_rejected(mutant):
    """discount 1 / log2(r + 1); ideal DCG over k ranks; precision over kmax; no clamp at 1; labels of row b under a permuted u_idx;
    a -1 entry counted as item 0: check_metrics raises on at least one input set of the GPU module"""
    rejected, n = [], 0
    for what, top, u, csr, ks in G.metrics_inputs():
        n += 1
        try:
            E.check_metrics(E.metrics_f32(top, u, csr, ks, mutant), top, u, csr, ks, what)
        except AssertionError as e:
            rejected.append(str(e))
    print(f'{mutant}: rejected on {len(rejected)} of {n} input sets; first: {rejected[0] if rejected else None}')
    assert rejected, f'{mutant}: no input set of the GPU tests sees it'


def test_restatement_without_a_mutant_is_the_same_function():
    what, top, u, csr, ks = [c for c in G.metrics_inputs() if 'Bu 257 kmax 20 permuted' in c[0] and len(c[4]) == 8][0]
    base = E.metrics_f32(top, u, csr, ks)
    assert np.array_equal(base.view(np.int32), E.metrics_f32(top, u, csr, ks).view(np.int32))
    for mutant in E.MUTANTS_METRICS:
        assert not np.array_equal(base.view(np.int32), E.metrics_f32(top, u, csr, ks, mutant).view(np.int32)), mutant


# ---- the evaluator's expectation ---------------------------------------------------------------------------------------------------
def test_the_evaluator_world_and_its_expectation():
    ds, calls, csr = G.evaluator_world()
    import scipy.sparse as sp
    lab = sp.csr_matrix(ds.user_sampling_matrix)[:, ds.items_in_split]
    lab.sort_indices()
    assert np.array_equal(lab.indptr, csr[0]) and np.array_equal(lab.indices, csr[1])           # what FullEvaluator._labels builds
    assert ds.user_sampling_matrix.nnz == len(csr[1]) + 300 and len(G.EVAL_KS) == 11
    assert sum(len(ids) for ids, _ in calls) == 320 and len(set(calls[0][0]) & set(calls[1][0])) == 20
    assert sum(int((top.numpy() < 0).any(axis=1).sum()) for _, top in calls) > 30
    per_user, coverage = G.evaluator_expectation(calls, csr)
    assert len(per_user) == 55 and len(coverage) == 11 and all(0 < c <= 1 for c in coverage.values())
    f, pr, rc = per_user['f_score@10'][0], per_user['precision@10'][0], per_user['recall@10'][0]
    assert (f[(pr + rc) == 0] == 0).all() and ((pr + rc) == 0).any() and np.allclose(f[pr > 0], 2 * pr[pr > 0] * rc[pr > 0] / (pr + rc)[pr > 0], rtol=1e-15)
    assert np.array_equal(per_user['hitrate@10'][0], (pr > 0).astype(np.float64))
