"""DirectAU without a GPU: the float64 restatement of the uniformity term (tests/directau_ref.py) against torch's pdist composition and its
autograd gradient, the numpy float32 restatement of the kernel's formula inside the derived bound, the alignment term on cosine logits,
the declared entries, the registry, the constructor's refusals and build_from_conf."""
import os
import re

import numpy as np
import pytest
import torch

import directau_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('sbr_uniformity_workspace', 'sbr_uniformity_fwd', 'sbr_uniformity_bwd', 'sbr_align_fwd', 'sbr_align_bwd')


def S():
    import sibrar_amd
    return sibrar_amd


@pytest.mark.parametrize('t', [0.5, 2.0])
@pytest.mark.parametrize('n', [2, 5, 70])
def test_float64_restatement_equals_the_pdist_composition_and_its_gradient(n, t):
    x = R.rows(n, 12, 1, unit=False, dup=0.0 if n == 2 else 0.3).astype(np.float64)
    if n > 2:
        assert len(np.unique(x, axis=0)) < n, 'the batch has duplicate rows'
    xt = torch.tensor(x, requires_grad=True)
    want = torch.pdist(xt).pow(2).mul(-t).exp().mean().log()
    want.backward()
    want = want.detach()
    loss, s = R.uniformity64(x, t)
    assert abs(loss - float(want)) <= 1e-12
    assert abs(s - float(torch.pdist(xt.detach()).pow(2).mul(-t).exp().sum())) <= 1e-12 * s
    assert float(np.abs(R.uniformity_grad64(x, t) - xt.grad.numpy()).max()) <= 1e-12
    assert float((R.uniformity_torch(xt.detach(), t) - want).abs()) <= 1e-12


@pytest.mark.parametrize('n, D, unit, t', [(2, 1, True, 2.0), (3, 31, True, 16.0), (65, 33, True, 2.0), (129, 64, False, 0.5),
                                           (200, 100, True, 16.0), (70, 256, False, 2.0)])
def test_float32_restatement_stays_inside_the_bound(n, D, unit, t):
    x = R.rows(n, D, 2, unit=unit, dup=0.3 if n > 3 else 0.0)
    loss64, s64 = R.uniformity64(x, t)
    loss32, s32 = R.uniformity32(x, t)
    assert abs(float(s32) - s64) <= R.s_rel(x, t) * s64
    assert abs(float(loss32) - loss64) <= R.loss_bound(x, t)
    err = np.abs(R.uniformity_grad32(x, t, s32).astype(np.float64) - R.uniformity_grad64(x, t))
    bound = R.grad_bound(x, t)
    assert bool((err <= bound).all()), f'worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}'
    print(f'n={n} D={D} t={t}: loss error {abs(float(loss32) - loss64):.3e} of {R.loss_bound(x, t):.3e}, gradient error {err.max():.3e} of '
          f'{bound.max():.3e}')


def test_two_identical_rows_and_two_orthogonal_rows():
    x = np.tile(R.rows(1, 16, 3), (2, 1))
    loss, s = R.uniformity32(x, 2.0)
    assert abs(float(s) - 1.0) <= R.s_rel(x, 2.0) and bool((R.uniformity_grad32(x, 2.0, s) == 0).all())
    e = np.eye(2, 8, dtype=np.float32)
    assert abs(R.uniformity64(e, 2.0)[0] + 4.0) <= 1e-12                      # d^2 = 2: loss = -2 t


def test_align_on_cosine_logits_is_the_mean_squared_distance():
    rng = np.random.default_rng(4)
    u, i = rng.standard_normal((37, 16)), rng.standard_normal((37, 4, 16))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    i /= np.linalg.norm(i, axis=-1, keepdims=True)
    logits = (u[:, None, :] * i).sum(-1)
    labels = np.zeros((37, 4))
    labels[:, 0] = 1
    want = ((u - i[:, 0]) ** 2).sum(-1).mean()
    assert abs(R.align64(logits, labels, 1 / 37) - want) <= 1e-12


def test_the_header_declares_the_entries_without_a_leading_dimension():
    text = open(os.path.join(ROOT, 'include', 'sibrar_hip.h')).read()
    text = re.sub(r'//[^\n]*', ' ', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))
    for e in ENTRIES:
        found = re.findall(r'\b' + e + r'\s*\(([^)]*)\)', text)
        assert len(found) == 1, e
        assert not any(re.fullmatch(r'(?:const\s+)?long\s+ld\w*', p.strip()) for p in found[0].split(',')), e
    assert 'int max_wg' in re.findall(r'\bsbr_uniformity_fwd\s*\(([^)]*)\)', text)[0]
    assert 'int max_wg' in re.findall(r'\bsbr_uniformity_bwd\s*\(([^)]*)\)', text)[0]


def test_registry_loss_enum_and_exports():
    Sm = S()
    assert Sm.ALGORITHMS['directau'] is Sm.DirectAU and issubclass(Sm.DirectAU, Sm.LightGCN)
    assert Sm.RecommenderSystemLossesEnum['align'].value is Sm.RecAlignmentLoss and issubclass(Sm.RecAlignmentLoss, Sm.RecommenderSystemLoss)
    assert Sm.ops.UNIFORMITY_MAX_D == 256
    for name in ('uniformity', 'UniformityFn', 'AlignLossFn'):
        assert hasattr(Sm.ops, name)
    assert [e.name for e in Sm.RecommenderSystemLossesEnum][:3] == ['bce', 'bpr', 'sampled_softmax']


def test_constructor_refusals_and_no_matrix_without_layers():
    Sm = S()
    net = Sm.DirectAU(50, 40)                                                    # n_layers = 0: no matrix, no graph
    assert net._graph is None and net.n_layers == 0 and (net.gamma, net.t, net.embedding_dim) == (1.0, 2.0, 64)
    assert sorted(net.state_dict()) == ['item_embeddings.weight', 'user_embeddings.weight']
    Sm.DirectAU(5, 6, embedding_dim=256, t=16.0, gamma=0.0)
    for kwargs in ({'embedding_dim': 0}, {'embedding_dim': 257}, {'gamma': -0.1}, {'t': 0.0}, {'t': -1.0}, {'t': 16.5}, {'n_layers': 2},
                   {'n_layers': -1}):
        with pytest.raises(ValueError):
            Sm.DirectAU(50, 40, **kwargs)
    m = np.zeros((50, 40))
    m[0, 0] = m[1, 3] = 1
    assert Sm.DirectAU(50, 40, n_layers=2, train_matrix=m)._graph is not None
    with pytest.raises(ValueError):
        Sm.DirectAU(49, 40, n_layers=2, train_matrix=m)
    with pytest.raises(ValueError):
        Sm.LightGCN(50, 40, None, n_layers=1)
    mf = Sm.SGDMatrixFactorization(50, 40, 64)
    net.load_state_dict(mf.state_dict())                                         # mf's keys
    assert torch.equal(net.user_embeddings.weight, mf.user_embeddings.weight)
    out = net.get_and_reset_other_loss()
    assert set(out) == {'reg_loss', 'uniform_u', 'uniform_i'} and float(out['reg_loss']) == 0.0


def test_build_from_conf():
    Sm = S()
    ds = Sm.SyntheticDataset(60, 50, 600, seed=1, n_negative_samples=3)
    net = Sm.ALGORITHMS['directau'].build_from_conf({'embedding_dim': 12, 'gamma': 0.5, 't': 3.0, 'n_layers': 2}, ds)
    assert (net.n_users, net.n_items, net.embedding_dim, net.gamma, net.t, net.n_layers) == (60, 50, 12, 0.5, 3.0, 2)
    assert tuple(net._graph.shape) == (60, 50)
    default = Sm.DirectAU.build_from_conf({}, ds)
    assert (default.embedding_dim, default.gamma, default.t, default.n_layers) == (64, 1.0, 2.0, 0) and default._graph is None
    loss = Sm.RecommenderSystemLoss.build_from_conf({'learn': {'rec_loss': 'align'}, 'dataset': {'n_negative_samples': 3}}, ds)
    assert isinstance(loss, Sm.RecAlignmentLoss) and loss.aggregator == 'mean'
