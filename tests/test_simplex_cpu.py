"""SimpleX without a GPU: the float64 formulas of tests/simplex_ref.py against float64 autograd and central finite differences; the float32
restatement of 'sbr_ccl_loss_fwd_bwd' and 'sbr_scatter_add_cos_rows_sorted' inside its own derived bound; the condition on the GPU tests'
inputs (no negative slot within 1e-3 of the margin, or exactly on it in the margin cases); the C ABI of the entries (with the workspace
query 'sbr_ccl_loss_workspace'); the constructor, the registry and the state_dict."""
import os
import re
from importlib import import_module

import numpy as np
import pytest
import torch

import simplex_ref as R

ENTRIES = ('sbr_ccl_loss_fwd_bwd', 'sbr_scatter_add_cos_rows_sorted', 'sbr_ccl_loss_workspace')
SMALL = [R.shape_case(3, 5, 2), R.shape_case(4, 5, 2), R.shape_case(68, 1, 2)] + [R.slot_case(k) for k in R.SLOT_CASES]


def S():
    import sibrar_amd
    return sibrar_amd


@pytest.mark.parametrize('case', range(len(SMALL)))
def test_direct_gradients_against_autograd_and_finite_differences(case):
    H32, V32, i, margin, negw = SMALL[case]
    margin, negw = R.f32(margin), R.f32(negw)
    r = R.direct(H32, V32, i, margin, negw)
    H = torch.from_numpy(H32.astype(np.float64)).requires_grad_(True)
    V = torch.from_numpy(V32.astype(np.float64)).requires_grad_(True)
    L, pos, neg, y = R.loss_torch(H, V, i, margin, negw)
    L.backward()
    assert abs(float(L.detach()) - r['loss']) <= 1e-14 * max(1., abs(r['loss'])) and np.allclose(y.detach().numpy(), r['y'], rtol=1e-13, atol=1e-15)
    scale = max(1., float(np.abs(r['dH']).max()), float(np.abs(r['dV']).max()))
    assert np.allclose(H.grad.numpy(), r['dH'], rtol=1e-10, atol=1e-13 * scale)
    assert np.allclose(V.grad.numpy(), r['dV'], rtol=1e-10, atol=1e-13 * scale)
    # central differences of the float64 loss on the rows that are not clamped (a clamped row has no gradient through its norm)
    rng = np.random.default_rng(case)
    Hd, Vd = H32.astype(np.float64), V32.astype(np.float64)
    for _ in range(12):
        which, step = rng.integers(0, 2), 1e-6
        M, G = (Hd, r['dH']) if which == 0 else (Vd, r['dV'])
        a, b = rng.integers(0, M.shape[0]), rng.integers(0, M.shape[1])
        if not M[a].any():
            continue
        up, dn = M.copy(), M.copy()
        up[a, b] += step
        dn[a, b] -= step
        f = lambda X: R.direct(X if which == 0 else Hd, X if which == 1 else Vd, i, margin, negw)['loss']
        fd = (f(up) - f(dn)) / (2 * step)
        assert abs(fd - G[a, b]) <= 1e-6 * max(1., abs(G[a, b])), (which, a, b, fd, G[a, b])


@pytest.mark.parametrize('case', range(len(SMALL)))
def test_float32_restatement_inside_its_own_bound(case):
    H32, V32, i, margin, negw = SMALL[case]
    ref = R.reference(H32, V32, i, margin, negw)
    got = R.ccl32(H32, V32, i, margin, negw)
    assert np.array_equal(got['coef_a'] != 0, ref['r']['g'] != 0), 'the active set is the reference\'s'
    got['dV'] = R.scatter_cos32(got['coef_a'], got['coef_s'], H32, V32, i)
    worst = R.worst_ratios(got, ref)
    print(worst)
    assert all(np.isfinite(v).all() for v in got.values())
    assert max(worst.values()) <= 1.0, worst
    assert max(worst.values()) > 0, 'float32 is not float64'


def test_restatement_details():
    a, c_ = np.float32(1 + 2.0 ** -12), np.float32(-(1 + 2.0 ** -11))                  # a * a = 1 + 2^-11 + 2^-24: the last bit is lost unfused
    assert R.fmaf32(a, a, c_) == np.float32(2.0 ** -24) and np.float32(a * a) + c_ == 0
    assert [R.geometry(D) for D in (1, 3, 4, 64, 68, 100, 256)] == [(1, 1, 1), (1, 4, 1), (4, 1, 1), (4, 16, 1), (4, 32, 1), (4, 32, 1), (4, 64, 1)]
    assert R.geometry(65) == (1, 64, 2) and R.geometry(255) == (1, 64, 4)
    x = np.random.default_rng(0).standard_normal((5, 68)).astype(np.float32)
    assert np.allclose(R.group_dot32(x, x), (x.astype(np.float64) ** 2).sum(1), rtol=1e-6)
    # rows that no slot names keep their contents; a sentinel slot adds nothing
    H32, V32, i, margin, negw = R.slot_case('outside')
    g = R.ccl32(H32, V32, i, margin, negw)
    dst = np.full(V32.shape, 7, dtype=np.float32)
    out = R.scatter_cos32(g['coef_a'], g['coef_s'], H32, V32, i, 0.5, dst)
    unnamed = np.setdiff1d(np.arange(V32.shape[0]), i[(i >= 0) & (i < V32.shape[0])])
    assert np.all(out[unnamed] == 7) and np.all(g['coef_a'][(i < 0) | (i >= V32.shape[0])] == 0)


def test_gpu_input_sets_keep_every_negative_away_from_the_margin():
    sets = [R.shape_case(*c) for c in R.SHAPE_CASES] + [R.slot_case(k) for k in R.SLOT_CASES]
    assert {c[0] for c in R.SHAPE_CASES} == {1, 3, 4, 64, 68, 256} and {c[1] for c in R.SHAPE_CASES} == {1, 5, 33} \
        and {c[2] for c in R.SHAPE_CASES} == {1, 2, 65, 130}
    for H, V, i, margin, negw in sets:
        assert 7 <= V.shape[0] <= 50 and -1 <= margin <= 1
        assert R.margin_gap(H, V, i, margin) >= R.GAP
        active = R.direct(H, V, i, R.f32(margin), R.f32(negw))['g'][:, 1:] != 0
        if H.shape[1] > 1 and active.size >= 10:
            assert active.any() and not active.all(), 'the set holds active and inactive negatives'
    for name, H, V, i, margin, negw, all_active in R.margin_cases():
        r = R.direct(H, V, i, R.f32(margin), R.f32(negw))
        d = np.abs(r['y'][:, 1:] - margin)
        assert np.all((d == 0) | (d >= R.GAP)), name
        assert bool((r['g'][:, 1:] != 0).all()) == all_active and (all_active or not (r['g'][:, 1:] != 0).any()), name
        if not all_active:
            assert (d == 0).any(), 'a score equals the margin'
            assert np.all(R.ccl32(H, V, i, margin, negw)['scores'][0, 1:] == 1), 'and does so in float32'
    # the whole model's batches (tests/test_hip_simplex.py), on the float64 representations
    for gamma_ in R.MODEL_GAMMAS:
        c = R.model_case(gamma_)
        _, y, h, _ = R.model_grads(c, torch.float64)
        assert R.margin_gap(h.numpy(), c['V'], c['i'], c['margin']) >= R.GAP and 7 in c['u']
    # the second group holds what it promises
    _, V, i, _, _ = R.slot_case('repeats')
    assert np.all(i[:, 2] == i[:, 0]) and np.all(i[:, 4] == i[:, 3])
    _, V, i, _, _ = R.slot_case('outside')
    assert (i == -1).any() and (i == V.shape[0]).any()
    H, V, i, _, _ = R.slot_case('zero_rows')
    assert not V[2].any() and not H[1].any() and (i[:, 0] == 2).any() and (i[:, 1:] == 2).any()


def test_the_header_declares_the_entries_and_the_walk_is_shared():
    lib = import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')
    protos = lib.parse_header()
    for e in ENTRIES:
        assert e in protos, f'{e} is not declared in include/sibrar_hip.h'
    assert protos['sbr_ccl_loss_fwd_bwd'][2][:3] == ['H', 'V', 'i_idxs'] and {'coef_a', 'coef_s'} <= set(protos['sbr_ccl_loss_fwd_bwd'][2])
    assert {'coef_s', 'V'} <= set(protos['sbr_scatter_add_cos_rows_sorted'][2])
    csrc = os.path.join(os.path.dirname(lib.LIB_PATH), '..', 'csrc')
    assert 'simplex.hip' in open(os.path.join(csrc, 'Makefile')).read()
    for f in ('ultragcn.hip', 'simplex.hip'):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "slot_rows.h"' in text and 'sbr_sorted_row_walk<' in text and 'sbr_sorted_segment(' in text, f
    for f in ('simplex.hip', 'slot_rows.h'):
        code = re.sub(r'//[^\n]*', '', open(os.path.join(csrc, f)).read())
        assert 'atomic' not in code.lower(), f'{f}: the new code has no atomics'


def test_constructor_registry_and_state_dict():
    Sm = S()
    assert Sm.ALGORITHMS['simplex'] is Sm.SimpleX and issubclass(Sm.SimpleX, Sm.LightGCN) and Sm.ops.CCL_MAX_D == 256
    ds = Sm.SyntheticDataset(50, 40, 700, seed=1, n_negative_samples=5)
    conf = {'embedding_dim': 12, 'gamma': 0.25, 'margin': 0.5, 'negative_weight': 20., 'init_std': 0.05}
    net = Sm.ALGORITHMS['simplex'].build_from_conf(conf, ds)
    assert (net.embedding_dim, net.gamma, net.margin, net.negative_weight, net.n_layers) == (12, 0.25, 0.5, 20., 0)
    assert 0.03 < float(net.item_embeddings.weight.detach().std()) < 0.07
    d = Sm.SimpleX.build_from_conf({}, ds)
    assert (d.embedding_dim, d.gamma, d.margin, d.negative_weight) == (64, 0.5, 0.9, 10.)
    assert float(d.user_embeddings.weight.detach().abs().max()) < 1e-3, 'init_std = 1e-4'
    assert list(d.state_dict()) == ['user_embeddings.weight', 'item_embeddings.weight', 'history_linear.weight']
    assert tuple(d.history_linear.weight.shape) == (64, 64) and d.history_linear.bias is None
    mf = Sm.SGDMatrixFactorization(50, 40, 64)
    before = d.history_linear.weight.detach().clone()
    missing = d.load_state_dict(mf.state_dict(), strict=False)
    assert list(missing.missing_keys) == ['history_linear.weight'] and not missing.unexpected_keys
    assert torch.equal(d.item_embeddings.weight, mf.item_embeddings.weight) and torch.equal(d.history_linear.weight, before)
    # the history matrix: X with rows scaled by 1 / d_u, out of the state_dict
    m = ds.user_sampling_matrix_train
    deg = np.diff(m.tocsr().indptr)
    assert tuple(d._history.shape) == (50, 40) and d._history.indices.numel() == m.nnz
    want = np.repeat((1. / np.maximum(deg, 1)).astype(np.float32), deg)
    assert np.array_equal(d._history.data.numpy(), want)
    valued = m.tocsr().astype(np.float32).copy()
    valued.data[0] = 2.
    for args, kwargs in (((50, 40, m), {'embedding_dim': 0}), ((50, 40, m), {'embedding_dim': 257}), ((50, 40, m), {'gamma': -0.1}),
                         ((50, 40, m), {'gamma': 1.5}), ((50, 40, m), {'margin': 1.5}), ((50, 40, m), {'margin': -1.5}),
                         ((50, 40, m), {'negative_weight': -1.}), ((50, 40, m), {'init_std': 0.}), ((49, 40, m), {}), ((50, 40, None), {}),
                         ((50, 40, valued), {})):
        with pytest.raises(ValueError, match='SimpleX'):
            Sm.SimpleX(*args, **kwargs)
    assert d.get_and_reset_other_loss().keys() == {'reg_loss', 'pos_loss', 'neg_loss'}
    assert all(float(v) == 0 for v in d.get_and_reset_other_loss().values())
    items_fn, users_fn, finish_fn = d.fused_score_transform()
    assert items_fn is Sm.ops.l2_normalize_rows and users_fn is Sm.ops.l2_normalize_rows and finish_fn is None
