"""SimpleX (simplex.py) on the GPU, on the 40 x 30 world of tests/simplex_ref.py (user 7 has an empty history): a training forward and
backward against the float64 model for all three parameters (both paths to the item table added) at gamma 0, 0.5 and 1, within 8 times
the error of the same network in torch float32 on the CPU; evaluation scores through ``forward``; the full-catalogue routes at
embedding_dim 64 against the float64 cosine ranking; optimizer steps that lower the loss; bit-identical deterministic fits; save and
load; the kept losses. Measured on an MI355X at gamma 0.5: scores 1.00e-07 against 1.27e-07 for float32 on the CPU, dV 1.26e-08 against
7.95e-09, dW 1.17e-08 against 9.80e-09 (8 x allowed). Reached entries: 'sbr_ccl_loss_fwd_bwd', 'sbr_scatter_add_cos_rows_sorted'."""
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import scorer_truth_util as T
import simplex_ref as R
from hip_testutil import DEV, S, _assert_bits

pytestmark = pytest.mark.gpu
ROUTE_C = 72.0        # scorer_truth_util's C = 64 for the product plus 8 for the float32 normalisation of both operands (tests/test_hip_deepmf.py)


def _mod(name):
    return import_module(S().ops.__name__.rsplit('.', 1)[0] + '.' + name)


def _net(c):
    net = S().SimpleX(40, 30, c['m'], embedding_dim=c['U'].shape[1], gamma=c['gamma'], margin=c['margin'], negative_weight=c['negative_weight'])
    net.load_state_dict({'user_embeddings.weight': torch.from_numpy(c['U']), 'item_embeddings.weight': torch.from_numpy(c['V']),
                         'history_linear.weight': torch.from_numpy(c['W'])})
    return net.to(DEV)


def _within(got, want, yard, what):
    err, allowed = float((got.double().cpu() - want).abs().max()), R.FACTOR * float((yard.double() - want).abs().max())
    print(f'{what}: error {err:.3e}, float32 on the CPU {allowed / R.FACTOR:.3e}, allowed {allowed:.3e}')
    assert err <= allowed, what


@pytest.mark.parametrize('gamma_', R.MODEL_GAMMAS)
def test_training_forward_and_backward_against_the_float64_model(gamma_):
    c = R.model_case(gamma_)
    L64, y64, h64, g64 = R.model_grads(c, torch.float64)
    L32, y32, h32, g32 = R.model_grads(c, torch.float32)
    net = _net(c).train()
    u, i = torch.from_numpy(c['u']).to(DEV), torch.from_numpy(c['i']).to(DEV)
    assert 7 in c['u'], 'the user with the empty history is in the batch'
    scores = net(u, i)
    assert scores.shape == i.shape and not scores.requires_grad
    other = net.get_and_reset_other_loss()
    assert set(other) == {'reg_loss', 'pos_loss', 'neg_loss'}
    (S().RecNoLoss(n_items=30).compute_loss(scores, None) + other['reg_loss']).backward()
    torch.cuda.synchronize()
    _within(scores, y64, y32, f'gamma {gamma_}: scores')
    L = float(other['reg_loss'].detach())
    print(f'gamma {gamma_}: loss {L:.7f} (float64 {L64:.7f}), error {abs(L - L64):.3e}, float32 on the CPU {abs(L32 - L64):.3e}')
    assert abs(L - L64) <= R.FACTOR * abs(L32 - L64) + 2 * R.U * abs(L64), 'the loss is a float32 scalar: two roundings of its own'
    assert abs(L - (float(other['pos_loss']) + R.f32(c['negative_weight']) * float(other['neg_loss']))) <= 4 * R.U * abs(L)
    params = {'U': net.user_embeddings.weight, 'V': net.item_embeddings.weight, 'W': net.history_linear.weight}
    for k, p in params.items():
        _within(p.grad, g64[k], g32[k], f'gamma {gamma_}: d{k}')
    assert float(g64['V'].abs().max()) > 0 and (gamma_ == 0.) == (float(g64['U'].abs().max()) == 0) and (gamma_ == 1.) == (float(g64['W'].abs().max()) == 0)
    # evaluation: the same cosines through forward, and the representation itself
    net.eval()
    with torch.no_grad():
        ev = net(u, i)
        h = net.get_user_representations(u)
    _within(ev, y64, y32, f'gamma {gamma_}: evaluation scores')
    _within(h, h64, h32, f'gamma {gamma_}: h')
    assert not h64[0].any() or gamma_ > 0, 'gamma 0: the user without history is represented by zero'


def _train(net, batch, steps, lr=1e-2):
    Sm = S()
    net.train()
    opt = Sm.FusedOptimizer(net, 'adam', lr, 0.)
    u, i = torch.from_numpy(batch[0]).to(DEV), torch.from_numpy(batch[1]).to(DEV)
    losses = []
    for _ in range(steps):
        scores = net(u, i)
        other = net.get_and_reset_other_loss()
        (Sm.RecNoLoss(n_items=30).compute_loss(scores, None) + other['reg_loss']).backward()
        opt.step()
        opt.zero_grad()
        losses.append(float(other['reg_loss']))
    torch.cuda.synchronize()
    return [v.detach().cpu() for v in net.state_dict().values()], losses


def test_steps_lower_the_loss_deterministic_fits_repeat_and_checkpoints_round_trip(tmp_path):
    Sm = S()
    c = R.model_case(0.5)
    batch = (c['u'], c['i'])
    prev = Sm.ops.set_deterministic(True)
    try:
        before = Sm.ops.nondeterministic_launches()
        net = _net(c)
        a = _train(net, batch, 6)
        b = _train(_net(c), batch, 6)
        assert Sm.ops.nondeterministic_launches() == before, 'a training step took an arrival-order path'
    finally:
        Sm.ops.set_deterministic(prev)
    print(f'losses {a[1]}')
    assert a[1][-1] < a[1][0], 'six Adam steps on one batch lower its loss'
    assert a[1] == b[1] and all(torch.equal(x, y) for x, y in zip(a[0], b[0]))
    assert not torch.equal(a[0][2], torch.from_numpy(c['W'])) and not torch.equal(a[0][1], torch.from_numpy(c['V']))
    zeros = net.get_and_reset_other_loss()
    assert set(zeros) == {'reg_loss', 'pos_loss', 'neg_loss'} and all(float(v) == 0 for v in zeros.values()), 'nothing was kept'
    net.save_model_to_path(str(tmp_path))
    back = Sm.SimpleX(40, 30, c['m'], embedding_dim=8).to(DEV)
    back.load_model_from_path(str(tmp_path))
    assert list(back.state_dict()) == ['user_embeddings.weight', 'item_embeddings.weight', 'history_linear.weight']
    for k, v in net.state_dict().items():
        _assert_bits(back.state_dict()[k].cpu(), v.cpu(), k)


def test_trainer_with_the_none_loss():
    Sm = S()
    prev = Sm.ops.is_deterministic()
    Sm.reproducible(5)
    try:
        ds = Sm.SyntheticDataset(50, 40, 700, seed=1, n_negative_samples=7)
        net = Sm.ALGORITHMS['simplex'].build_from_conf({'embedding_dim': 16, 'init_std': 0.1, 'margin': 0.4, 'negative_weight': 5.}, ds)
        loss = Sm.RecommenderSystemLoss.build_from_conf({'learn': {'rec_loss': 'none'}, 'dataset': {'n_negative_samples': 7}}, ds)
        loader = Sm.NegativeSamplingDataLoader(ds, batch_size=64, shuffle=True)
        tr = Sm.Trainer(net, loader, None, loss, {'learn': {'lr': 1e-2, 'wd': 0., 'optimizer': 'adam'}, 'run_settings': {'device': DEV}})
        assert tr.fused is None
        e0, e1 = tr.train(), tr.train()
    finally:
        Sm.ops.set_deterministic(prev)
    print(f'epoch 0 {e0}\nepoch 1 {e1}')
    assert {'train/loss', 'train/rec_loss', 'train/reg_loss', 'train/pos_loss', 'train/neg_loss'} <= set(e0), set(e0)
    assert all(np.isfinite(v) for v in e0.values()) and e0['train/rec_loss'] == 0.0 and e0['train/loss'] == e0['train/reg_loss'] > 0
    assert e1['train/loss'] < e0['train/loss']


@pytest.fixture(scope='module')
def eval_world():
    Sm = S()
    ds = Sm.SyntheticDataset(600, 500, 12000, seed=4, n_negative_samples=3, holdout_per_user=1)
    gen = torch.Generator().manual_seed(12)
    net = Sm.SimpleX(600, 500, ds.user_sampling_matrix_train, embedding_dim=64)
    net.load_state_dict({'user_embeddings.weight': torch.randn(600, 64, generator=gen) * 0.5,
                         'item_embeddings.weight': torch.randn(500, 64, generator=gen) * torch.logspace(-1, 1, 500)[:, None],
                         'history_linear.weight': torch.randn(64, 64, generator=gen) / 8})
    net = net.to(DEV).eval()
    view = ds.eval_view()
    with torch.no_grad():
        h = net.get_user_representations(torch.arange(600, device=DEV)).double()
        v = net.get_item_representations(torch.arange(500, device=DEV)).double()
    hn, vn = h / h.norm(dim=1, keepdim=True).clamp(min=1e-8), v / v.norm(dim=1, keepdim=True).clamp(min=1e-8)
    excluded = torch.from_numpy(view.exclude_data.toarray() != 0).to(DEV)
    return SimpleNamespace(net=net, view=view, masked=(hn @ vn.t()).masked_fill(excluded, -float('inf')), raw=(h @ v.t()).masked_fill(excluded, -float('inf')),
                           tol=ROUTE_C * 2.0 ** -24 * (hn.abs() @ vn.abs().t()))


@pytest.mark.parametrize('scorer', ['fp32', 'fp32_fused'])
def test_full_catalogue_evaluation_ranks_by_the_cosine_on_either_route(eval_world, scorer):
    """embedding_dim 64: the fp32_fused route is taken through ``fused_score_transform``, and both routes give the float64 ranking of the
    cosine up to near-ties (tests/scorer_truth_util.py); the item norms span two decades, so a dot-product ranking would differ"""
    w, Sm = eval_world, S()
    ev = Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=(1, 10, 20)), dataset=w.view)
    got = []
    L = _mod('_lib')
    L.CALL_LOG = []
    try:
        Sm.evaluation._score_split(w.net, type('L', (), {'dataset': w.view, 'batch_size': 256})(), ev, DEV, scorer, 256, False, 32,
                                   lambda s, u_, v, ix: got.append((v, ix)))
        names = [n for n, _ in L.CALL_LOG]
    finally:
        L.CALL_LOG = None
    assert any(n.startswith('sbr_score_topk_f32s') for n in names) == (scorer == 'fp32_fused'), set(names)
    assert 'sbr_ccl_loss_fwd_bwd' not in names, 'evaluation does not need the loss'
    lists = (torch.cat([g[0] for g in got]), torch.cat([g[1] for g in got]))
    T.check_against_truth(lists, torch.arange(600, device=DEV), w.masked, w.tol, 20, what=scorer)
    by_dot = torch.topk(w.raw, 20, dim=1).indices
    assert int((by_dot[:, 0] != lists[1][:, 0]).sum()) > 100, 'the inputs tell the cosine from the dot product'
