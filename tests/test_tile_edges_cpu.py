"""The CPU side of tests/test_hip_tile_edges.py: every shape and seed of tests/tile_edges_cases.py meets the preconditions under which its
discrete decisions are the same in fp32 and float64 (arg-min margins, near-tie share, clamp and ReLU kinks, no empty anchor), the
references are self-consistent, and each reach shape really reaches its branch under the restated host rules."""
import pytest
import torch

import tile_edges_cases as TC
from tile_edges_cases import case_id


def S():
    import sibrar_amd
    return sibrar_amd


def test_restated_constants_are_the_mirrored_ones():
    ops = S().ops
    assert TC.T64_T == ops.ANCHOR_TILE == ops.CLUSTER_TILE == 64 and TC.T64_MAX_WG == ops.ANCHOR_MAX_WG == 1024
    assert TC.T64_MAX_N == ops.PROTO_MAX_P == ops.ANCHOR_MAX_K == ops.CLUSTER_MAX_C
    assert TC.NEAR_TIE_CAP == 0.03 and TC.KAPPA == 3.0 and TC.REL_FLOOR == 1e-7


def test_the_lists_cover_the_edges():
    """every edge value of R, D and N, every register-block count, both chunk edges, rows == NULL and a lookup, both loss forms,
    fan in {1, 3} with and without widx, top in {1, a middle value, C}"""
    Rs, Ds, Ns = ({c[n] for c in TC.BASE} for n in range(3))
    assert Rs == {1, 63, 64, 65, 129} and Ds >= {1, 31, 32, 33, 64, 65, 512} and Ns == {2, 63, 64, 65, 129, 192, 193, 256}
    assert {TC.tiles(n) for n in Ns} == {1, 2, 3, 4}
    assert {c[3] for c in TC.SIM_CASES} == {True, False}
    assert {(c[3], c[4]) for c in TC.SCORE_CASES if not c[6]} >= {(0, False), (1, True), (1, False), (3, True), (3, False)}
    assert {c[5] for c in TC.SCORE_CASES} == {True, False} and {c[4] for c in TC.ANCHOR_CASES} == {True, False}
    assert {c[3] for c in TC.ANCHOR_CASES} == {True, False}
    tops = [(c[2], c[3]) for c in TC.CLUSTER_CASES]
    assert any(t == 1 for _, t in tops) and any(t == C for C, t in tops) and any(1 < t < C for C, t in tops)
    assert {TC.tiles(C) for C, t in tops if t == C} >= {1, 2, 4} and {TC.tiles(C) for C, t in tops if 1 < t < C} >= {1, 3, 4}


def _owners(n_tiles, wgs):
    """tiles per workgroup of a grid-stride pass"""
    return [len(range(b, n_tiles, wgs)) for b in range(wgs)]


def test_reach_shapes_reach_their_branches():
    R, D, N = TC.REACH_FWD
    assert TC.tiles(R) == 1026 and R - 64 * 1025 == 1
    own = _owners(TC.tiles(R), TC.t64_wgs(R))
    assert len(own) == TC.T64_MAX_WG and own[:3] == [2, 2, 1] and sum(own) == 1026          # anchor_mix, cluster_affil
    assert TC.t64_wgs(R, TC.PS_MAX_WG) == 256 and min(_owners(1026, 256)) == 4                # ProtoMF: every workgroup loops
    assert TC.t64_wgs(R, TC.PC_MAX_WG) == 1026                                                # ProtoMFs at this shape: no loop, hence:
    R2 = TC.REACH_FWD_SCORE[0]
    assert _owners(TC.tiles(R2), TC.t64_wgs(R2, TC.PC_MAX_WG))[:2] == [2, 1] and TC.t64_wgs(R2 - 1, TC.PC_MAX_WG) == TC.tiles(R2 - 1)
    R, D, N = TC.REACH_BWD
    assert TC.tiles(R) == 130 and R - 64 * 129 == 1
    assert TC.am_splits(R, D, N) == 128 and _owners(130, 128)[:3] == [2, 2, 1]
    assert TC.ca_splits(R, D, N) == 127 and _owners(130, 127)[:4] == [2, 2, 2, 1]
    assert TC.am_splits(128 * 64, D, N) == 128 == TC.tiles(128 * 64)                          # one row tile fewer: no second tile
    assert TC.pc_splits(R, D, N) == 8
    for R, D, N in TC.BASE:                                                                   # the small shapes: one tile per workgroup
        assert TC.t64_wgs(R) == TC.tiles(R) == TC.am_splits(R, D, N) == TC.ca_splits(R, D, N) <= 3


def test_restated_workspace_sizes_are_consistent_with_the_rules():
    R, D, N = TC.REACH_BWD
    assert TC.ws_bytes('sbr_anchor_mix_workspace', R, D, N, True) == 128 * N * D * 4 == 64 << 20
    assert TC.ws_bytes('sbr_cluster_affil_workspace', R, D, N, True) == 2048 + 127 * N * (D + 1) * 4
    assert TC.ws_bytes('sbr_proto_sim_workspace', *TC.REACH_FWD, False) == 256 * 8 + 2048 + 256 * 3 * 8


@pytest.mark.parametrize('case', TC.SIM_CASES, ids=case_id)
def test_proto_sim_preconditions(case):
    R, D, P, lookup, _ = case
    inp = TC.sim_inputs(R, D, P, lookup)
    TC.sim_precondition(inp)
    if lookup:
        assert sorted(inp['rows'].tolist()) == list(range(R)), 'a permutation: equal rows would tie exactly in the column minimum'
    if R <= 129:
        ref = TC.sim_ref(inp, torch.float64)
        e = TC.gathered(inp).double()
        assert torch.equal(ref['row_best'].long(), (2 - ref['sim']).argmin(dim=1)) or D == 1
        assert torch.allclose(ref['cos_raw'] * ref['row_stat'][:, :1] * ref['proto_stat'][:, 0], e @ inp['protos'].double().T, atol=1e-12)


@pytest.mark.parametrize('case', TC.SCORE_CASES, ids=case_id)
def test_proto_score_preconditions(case):
    R, D, P, fan, with_widx, lookup, fwd_only = case
    inp = TC.score_inputs(R, D, P, fan, with_widx, lookup)
    if not fwd_only:                                  # the forward clamp and ReLU are continuous: only a gradient can flip at a kink
        TC.score_precondition(inp)
    assert (inp['rows'] is not None) == lookup and (inp['widx'] is not None) == (with_widx and fan > 0)
    if lookup and R >= 4:
        assert len(set(inp['rows'].tolist())) == R - 2, 'two duplicates'


@pytest.mark.parametrize('case', TC.ANCHOR_CASES, ids=case_id)
def test_anchor_mix_preconditions(case):
    R, D, K, loss, lookup, _ = case
    TC.anchor_precondition(TC.anchor_inputs(R, D, K, lookup))


@pytest.mark.parametrize('case', TC.CLUSTER_CASES, ids=case_id)
def test_cluster_affil_preconditions(case):
    R, D, C, top, _ = case
    inp = TC.cluster_inputs(R, D, C, top)
    share = TC.cluster_precondition(inp)
    print(f'near-tie rows left out at {case}: {share:.4f}')
    TC.logit_precondition(TC.logit_inputs(R, C, top))
    if R <= 129:
        ref = TC.cluster_ref(inp, torch.float64)
        assert bool(((ref['x'] != 0).sum(dim=1) == top).all())
        bits = ref['mask'].to(torch.int32)
        assert bool(((bits & 1) + ((bits >> 1) & 1) + ((bits >> 2) & 1) + ((bits >> 3) & 1)).sum(dim=1).eq(top).all()) and int(bits.max()) < 16
