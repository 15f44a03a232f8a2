"""UltraGCN without a GPU: the restatements of tests/ultragcn_ref.py against brute force and float64 autograd, on cases that hold exact value
ties; the C ABI of the three entries ('sbr_cooc_weight_topk', 'sbr_ultragcn_loss_fwd_bwd', 'sbr_scatter_add_scaled_rows_sorted' and the
workspace query 'sbr_ultragcn_loss_workspace') parses from the header; the registry, the configuration and ``rec_loss: none``."""
import os
import re

import numpy as np
import pytest
import torch

import ultragcn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('sbr_cooc_weight_topk', 'sbr_ultragcn_loss_fwd_bwd', 'sbr_scatter_add_scaled_rows_sorted', 'sbr_ultragcn_loss_workspace')


def S():
    import sibrar_amd
    return sibrar_amd


def test_g_is_the_row_sum_of_the_dense_gram_matrix():
    x = R.matrix(40, 23, 0.2, seed=1, empty_items=(4,))
    d = R.dense01(x)
    G = d.T @ d
    d_u, d_i, g = R.degrees(x)
    assert np.array_equal(g, G.sum(axis=1)) and np.array_equal(d_i, np.diag(G)) and np.array_equal(d_u, d.sum(axis=1))
    assert g[4] == 0 and d_i[4] == 0
    bu, bi, row, col = R.scales64(x)
    assert row[4] == 0 and col[4] == 1 and bi[4] == 1 and np.all(np.isfinite(np.concatenate([bu, bi, row, col])))
    om, _ = R.omega64(x)
    assert np.allclose(om, G * (np.sqrt(g + 1.) / np.maximum(g, 1))[:, None] / np.sqrt(g + 1.)[None, :], rtol=1e-15)


@pytest.mark.parametrize('shape,k,include_self', [((40, 23), 5, True), ((40, 23), 5, False), ((65, 33), 10, True), ((30, 12), 64, True)])
def test_lists_against_a_brute_force_dense_sort(shape, k, include_self):
    x = R.matrix(*shape, 0.2, seed=2, empty_items=(3,))
    bu, bi, row, col = R.scales32(x)
    v, G = R.values32(x, row, col)
    assert R.has_value_tie(v, G), 'the case must hold an exact value tie, or the index rule is not exercised'
    idx, val, length = R.select(v, G, k, include_self)
    brute = R.brute_force_lists(v, G, k, include_self)
    for i, want in enumerate(brute):
        assert length[i] == len(want) and idx[i, :length[i]].tolist() == want, f'row {i}'
        assert np.all(idx[i, length[i]:] == -1) and np.all(val[i, length[i]:] == 0), f'row {i}: padding'
        assert np.array_equal(val[i, :length[i]], v[i, want])
        if include_self and G[i, i] > 0:
            assert i in want or len(want) == k
    assert length[3] == 0, 'an item without users has an empty list'
    m = shape[1]
    assert length[m - 1] == (2 if include_self else 1) and length[m - 1] < k, 'the lonely pair: fewer candidates than k'
    # the float32 values are within 2 u of the float64 product of the same scales
    om, _ = R.omega64(x, row, col)
    assert np.all(np.abs(v.astype(np.float64) - om) <= R.gamma(2) * om)
    # rows=(r0, r1) of the restatement is the whole, cut
    part = R.select(v, G, k, include_self, rows=(5, 9))
    assert np.array_equal(part[0][5:9], idx[5:9]) and np.all(part[2][:5] == 0) and np.all(part[2][9:] == 0)


@pytest.mark.parametrize('D,B,N,K', [(3, 5, 2, 3), (8, 9, 7, 4)])
def test_analytic_coef_and_dub_against_float64_autograd(D, B, N, K):
    c = R.loss_case(D, B, N, K, big=False)
    Ub = torch.from_numpy(c['Ub'].astype(np.float64)).requires_grad_(True)
    V = torch.from_numpy(c['V'].astype(np.float64)).requires_grad_(True)
    r = R.loss_torch(Ub, V, c['u'], c['i'], c['beta_u'], c['beta_i'], c['nbr_idx'], c['nbr_val'], c['nbr_len'], R.SCALARS)
    s = r['scores'].detach().clone().requires_grad_(True)
    # dL/ds by autograd on the scores alone
    w1, w2, w3, w4, negw, lam = R.SCALARS
    terms = r['w'].detach() * torch.nn.functional.softplus(r['sgn'] * s) * r['mask']
    (terms[:, 0].sum() + negw * terms[:, 1:1 + N].sum() / N + lam * terms[:, 1 + N:].sum()).backward()
    coef, _ = R.analytic(r, R.SCALARS)
    assert torch.allclose(coef, s.grad, rtol=1e-12, atol=1e-15)
    assert bool((coef[~r['mask']] == 0).all()) and int((~r['mask']).sum()) > 0, 'padded slots carry no coefficient'
    r['loss'].backward()
    items = torch.from_numpy(np.where(r['items'] >= 0, r['items'], 0))
    dub = torch.einsum('bc,bcd->bd', coef, V.detach()[items])
    assert torch.allclose(dub, Ub.grad, rtol=1e-11, atol=1e-14)
    dv = torch.zeros_like(V).index_add_(0, items.reshape(-1), (coef[:, :, None] * Ub.detach()[:, None, :]).reshape(-1, D))
    assert torch.allclose(dv, V.grad, rtol=1e-11, atol=1e-14)
    # the case repeats what the kernel must get right: users, positives, an item that is positive, negative and neighbour at once
    assert len(set(c['u'].tolist())) < B and len(set(c['i'][:, 0].tolist())) < B
    it = r['items']
    assert any(it[b, 0] in it[b, 1:1 + N] and it[b, 0] in it[b, 1 + N:] for b in range(B))
    # the order oracle agrees with float64 to rounding, and fmaf32 is a fused operation
    ref = R.reference(c['Ub'], c['V'], c['u'], c['i'], c['beta_u'], c['beta_i'], c['nbr_idx'], c['nbr_val'], c['nbr_len'], R.SCALARS)
    dv32 = R.scatter_ordered32(ref['coef'][0].astype(np.float32), c['Ub'], ref['items'], c['V'].shape[0])
    assert np.all(np.abs(dv32 - ref['dV'][0]) <= 4 * (B * (1 + N + K)) * R.U * (np.abs(ref['dV'][0]).max() + 1))
    a, c_ = np.float32(1 + 2.0 ** -12), np.float32(-(1 + 2.0 ** -11))                  # a * a = 1 + 2^-11 + 2^-24: the last bit is lost unfused
    assert R.fmaf32(a, a, c_) == np.float32(2.0 ** -24) and np.float32(a * a) + c_ == 0


def test_the_header_declares_the_entries_and_the_makefile_builds_them():
    Sm = S()
    from importlib import import_module
    lib = import_module(Sm.ops.__name__.rsplit('.', 1)[0] + '._lib')
    protos = lib.parse_header()
    for e in ENTRIES:
        assert e in protos, f'{e} is not declared in include/sibrar_hip.h'
    for e in ENTRIES[:3]:
        assert not any(re.fullmatch(r'ld\w*', n) for n in protos[e][2]), f'{e} takes a leading dimension'
    assert protos['sbr_ultragcn_loss_fwd_bwd'][2][:3] == ['Ub', 'V', 'u_idxs'] and 'coef' in protos['sbr_ultragcn_loss_fwd_bwd'][2]
    assert 'ultragcn.hip' in open(os.path.join(os.path.dirname(lib.LIB_PATH), '..', 'csrc', 'Makefile')).read()
    csrc = os.path.join(os.path.dirname(lib.LIB_PATH), '..', 'csrc')
    for f in ('knn.hip', 'ultragcn.hip'):
        assert '#include "cooc_topk.h"' in open(os.path.join(csrc, f)).read(), f'{f} does not share the selection header'


def test_registry_configuration_and_the_none_loss():
    Sm = S()
    assert Sm.ALGORITHMS['ultragcn'] is Sm.UltraGCN and issubclass(Sm.UltraGCN, Sm.LightGCN)
    assert Sm.RecommenderSystemLossesEnum['none'].value is Sm.RecNoLoss and issubclass(Sm.RecNoLoss, Sm.RecommenderSystemLoss)
    ds = Sm.SyntheticDataset(50, 40, 700, seed=1, n_negative_samples=5)
    loss = Sm.RecommenderSystemLoss.build_from_conf({'learn': {'rec_loss': 'none'}, 'dataset': {'n_negative_samples': 5}}, ds)
    z = loss.compute_loss(torch.zeros(3, 6), torch.zeros(3, 6))
    assert isinstance(loss, Sm.RecNoLoss) and z.shape == () and float(z) == 0.0
    conf = {'embedding_dim': 12, 'n_neighbors': 7, 'w1': 1e-3, 'w2': 0.5, 'w3': 1e-4, 'w4': 0.25, 'negative_weight': 20., 'lam': 1e-2,
            'init_std': 0.05}
    net = Sm.ALGORITHMS['ultragcn'].build_from_conf(conf, ds)
    assert (net.embedding_dim, net.n_neighbors, net.w1, net.w2, net.w3, net.w4, net.negative_weight, net.lam) == \
        (12, 7, 1e-3, 0.5, 1e-4, 0.25, 20., 1e-2)
    assert 0.03 < float(net.item_embeddings.weight.detach().std()) < 0.07
    d = Sm.UltraGCN.build_from_conf({}, ds)
    assert (d.embedding_dim, d.n_neighbors, d.w1, d.w2, d.w3, d.w4, d.negative_weight, d.lam) == (64, 10, 1e-6, 1., 1e-6, 1., 300., 5e-4)
    assert float(d.user_embeddings.weight.abs().max()) < 1e-3, 'init_std = 1e-4'
    assert sorted(d.state_dict()) == ['item_embeddings.weight', 'user_embeddings.weight']
    mf = Sm.SGDMatrixFactorization(50, 40, 64)
    d.load_state_dict(mf.state_dict())
    assert torch.equal(d.item_embeddings.weight, mf.item_embeddings.weight)
    m = ds.user_sampling_matrix_train
    for kwargs in ({'embedding_dim': 0}, {'embedding_dim': 257}, {'n_neighbors': 0}, {'n_neighbors': 65}, {'lam': -1.}, {'init_std': 0.}):
        with pytest.raises(ValueError):
            Sm.UltraGCN(50, 40, m, **kwargs)
    with pytest.raises(ValueError):
        Sm.UltraGCN(49, 40, m)
    with pytest.raises(ValueError):
        Sm.UltraGCN(50, 40, None)
    assert d.get_and_reset_other_loss().keys() == {'reg_loss', 'pos_loss', 'neg_loss', 'nbr_loss'}
