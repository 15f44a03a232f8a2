"""NeuMF (neumf.py) on the GPU, on the 40 x 30 world of tests/neumf_ref.py: a training forward and backward under bce against the float64
model for the full model, plain GMF (L = 0) and the MLP model (Dg = 0), within 8 times the error of the same network in torch float32 on
the CPU; evaluation-mode ``forward`` and ``combine`` on all items within the kernel's derived bound; the full-catalogue evaluation with
``scorer='fp32'`` giving exactly the float64 top-10 lists (the condition is checked in tests/test_neumf_cpu.py); plain GMF at Dg = 64 on
the fp32_fused route; optimizer steps that lower the loss; bit-identical deterministic fits; save and load; ``load_pretrained``.
Reached entries: 'sbr_neumf_score_all', 'sbr_neumf_score_pairs'."""
from importlib import import_module

import numpy as np
import pytest
import torch

import neumf_ref as R
from hip_testutil import DEV, S, _assert_bits

pytestmark = pytest.mark.gpu


def _mod(name):
    return import_module(S().ops.__name__.rsplit('.', 1)[0] + '.' + name)


def _net(cfg, p):
    net = S().NeuMF(R.N_USERS, R.N_ITEMS, **cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    return net.to(DEV)


def _within(got, want, yard, what):
    err, allowed = float((got.double().cpu() - want).abs().max()), R.FACTOR * float((yard.double() - want).abs().max())
    print(f'{what}: error {err:.3e}, float32 on the CPU {allowed / R.FACTOR:.3e}, allowed {allowed:.3e}')
    assert err <= allowed, what


def _bce():
    return S().RecBinaryCrossEntropy(n_items=R.N_ITEMS, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=5)


@pytest.mark.parametrize('name', list(R.CONFIGS))
def test_training_forward_and_backward_under_bce_against_the_float64_model(name):
    cfg = R.CONFIGS[name]
    p = R.params(seed=3, **cfg)
    u, i, labels = R.batch()
    L64, y64, g64 = R.model_grads(p, u, i, labels, torch.float64)
    L32, y32, g32 = R.model_grads(p, u, i, labels, torch.float32)
    net = _net(cfg, p).train()
    ud, idv = torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV)
    y = net(ud, idv)
    assert y.shape == idv.shape and y.requires_grad
    other = net.get_and_reset_other_loss()
    assert set(other) == {'reg_loss'} and float(other['reg_loss']) == 0.
    loss = _bce().compute_loss(y, labels.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    _within(y.detach(), y64, y32, f'{name}: logits')
    # the mean of terms that are 1-Lipschitz in their logit moves by no more than the largest logit error; the scalar's own roundings beside it
    assert abs(float(loss) - L64) <= float((y.detach().double().cpu() - y64).abs().max()) + 4 * R.U * abs(L64)
    grads = dict(net.named_parameters())
    assert sorted(grads) == sorted(g64)
    for k in g64:
        assert float(g64[k].abs().max()) > 0, k
        _within(grads[k].grad, g64[k], g32[k], f'{name}: d {k}')


@pytest.mark.parametrize('name', list(R.CONFIGS))
def test_evaluation_forward_and_combine_within_the_kernel_bound(name):
    cfg = R.CONFIGS[name]
    p = R.params(seed=4, **cfg)
    net = _net(cfg, p).eval()
    u, i, _ = R.batch()
    ud, idv = torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV)
    lib = _mod('_lib')
    lib.CALL_LOG = []
    try:
        with torch.no_grad():
            ev = net(ud, idv)
            users, items = torch.arange(R.N_USERS, device=DEV), torch.arange(R.N_ITEMS, device=DEV)
            ur, ir = net.get_user_representations(users), net.get_item_representations(items)
            full = net.combine_user_item_representations(ur, ir)
            shard = net.combine_user_item_representations(ur[5:23], ir[7:])
        names = [n for n, _ in lib.CALL_LOG]
    finally:
        lib.CALL_LOG = None
    h1 = cfg['mlp_layers'][0] if cfg['mlp_layers'] else 0
    assert ur.shape == (R.N_USERS, h1 + cfg['gmf_dim']) and ir.shape == (R.N_ITEMS, h1 + cfg['gmf_dim'])
    assert ('sbr_neumf_score_all' in names) == bool(cfg['mlp_layers']) and ('sbr_neumf_score_pairs' in names) == bool(cfg['mlp_layers'])
    for got, (want, bound), what in ((ev, R.model_bound(p, u, i), 'forward'),
                                     (full, R.model_bound(p, np.arange(R.N_USERS), np.arange(R.N_ITEMS)), 'combine on all items')):
        ratio = float(((got.double().cpu() - want).abs() / bound).max())
        print(f'{name}: {what}: largest error / bound {ratio:.3f}')
        assert got.shape == want.shape and ratio <= 1., (name, what, ratio)
    _assert_bits(shard.cpu(), full[5:23, 7:].cpu(), 'a user chunk against an item shard')


def _lists(net, view, scorer, k):
    Sm = S()
    ev = Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=(1, k)), dataset=view)
    got = []
    lib = _mod('_lib')
    lib.CALL_LOG = []
    try:
        Sm.evaluation._score_split(net, type('L', (), {'dataset': view, 'batch_size': 16})(), ev, DEV, scorer, 16, False, 32,
                                   lambda s, u_, v, ix: got.append((v, ix)))
        names = [n for n, _ in lib.CALL_LOG]
    finally:
        lib.CALL_LOG = None
    return torch.cat([g[0] for g in got]), torch.cat([g[1] for g in got]), names


def test_full_catalogue_evaluation_gives_the_float64_top_10_lists():
    Sm = S()
    ds, view, p, y, e = R.eval_truth(Sm)
    left_out, want = R.left_out_users(y, e)
    assert left_out == []
    net = _net(R.CONFIGS['full'], p).eval()
    val, idx, names = _lists(net, view, 'fp32', R.EVAL_K)
    assert names.count('sbr_neumf_score_all') == 3, 'one launch per chunk of 16 users'
    assert torch.equal(idx.cpu().long(), want), 'exactly the float64 lists'
    assert float((val.double().cpu() - torch.gather(y, 1, want)).abs().div(torch.gather(e, 1, want)).max()) <= 1.
    # the fused routes are not offered a score that is no dot product: the same lists by the same kernel
    val2, idx2, names2 = _lists(net, view, 'fp32_fused', R.EVAL_K)
    assert 'sbr_neumf_score_all' in names2 and not any(n.startswith('sbr_score_topk') for n in names2)
    assert torch.equal(idx2, idx) and torch.equal(val2, val)
    metrics = Sm.evaluate_recommender_algorithm(net, type('L', (), {'dataset': view, 'batch_size': 16})(),
                                                Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=(1, R.EVAL_K)), dataset=view), device=DEV,
                                                scorer='fp32')
    assert all(np.isfinite(v) for v in metrics.values())


def test_plain_gmf_at_64_reaches_the_fused_scorer_with_the_same_lists():
    Sm = S()
    ds, view, _, _, _ = R.eval_truth(Sm)
    cfg = dict(gmf_dim=64, mlp_dim=0, mlp_layers=())
    net = _net(cfg, R.params(seed=9, scale=1.0, **cfg)).eval()
    val, idx, names = _lists(net, view, 'fp32', R.EVAL_K)
    valf, idxf, namesf = _lists(net, view, 'fp32_fused', R.EVAL_K)
    assert any(n.startswith('sbr_score_topk_f32s') for n in namesf) and not any(n.startswith('sbr_score_topk_f32s') for n in names)
    assert torch.equal(idx.long(), idxf.long())
    assert float((val - valf).abs().max()) <= 64 * 72 * R.U * float(val.abs().max()), 'out_bias is added on both routes'


def _train(net, batch, steps, lr=1e-2):
    Sm = S()
    net.train()
    opt = Sm.FusedOptimizer(net, 'adam', lr, 0.)
    u, i, labels = torch.from_numpy(batch[0]).to(DEV), torch.from_numpy(batch[1]).to(DEV), batch[2].to(DEV)
    losses = []
    for _ in range(steps):
        loss = _bce().compute_loss(net(u, i), labels)
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(float(loss))
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in net.state_dict().items()}, losses


def test_steps_lower_the_loss_deterministic_fits_repeat_and_checkpoints_round_trip(tmp_path):
    Sm = S()
    # widths in multiples of 4: the bias gradient's column sum (sbr_colsum) has its fixed-order form only there, and raises otherwise
    cfg, batch = dict(gmf_dim=4, mlp_dim=8, mlp_layers=(8, 4)), R.batch()
    p = R.params(seed=5, **cfg)
    prev = Sm.ops.set_deterministic(True)
    try:
        before = Sm.ops.nondeterministic_launches()
        net = _net(cfg, p)
        a = _train(net, batch, 6)
        b = _train(_net(cfg, p), batch, 6)
        assert Sm.ops.nondeterministic_launches() == before, 'a training step took an arrival-order path'
    finally:
        Sm.ops.set_deterministic(prev)
    print(f'losses {a[1]}')
    assert a[1][-1] < a[1][0], 'six Adam steps on one batch lower its loss'
    assert a[1] == b[1] and all(torch.equal(a[0][k], b[0][k]) for k in a[0])
    assert all(not torch.equal(a[0][k], torch.from_numpy(p[k])) for k in p), 'every parameter moved'
    net.save_model_to_path(str(tmp_path))
    back = Sm.NeuMF(R.N_USERS, R.N_ITEMS, **cfg).to(DEV)
    back.load_model_from_path(str(tmp_path))
    assert sorted(back.state_dict()) == sorted(R.state_keys(**cfg))
    for k, v in net.state_dict().items():
        _assert_bits(back.state_dict()[k].cpu(), v.cpu(), k)


@pytest.mark.parametrize('alpha', [0.5, 0.25])
def test_load_pretrained_reproduces_the_mix_of_the_two_models(alpha):
    pg, pm = R.params(seed=6, **R.CONFIGS['gmf']), R.params(seed=7, **R.CONFIGS['mlp'])
    gmf, mlp = _net(R.CONFIGS['gmf'], pg), _net(R.CONFIGS['mlp'], pm)
    net = S().NeuMF(R.N_USERS, R.N_ITEMS, **R.CONFIGS['full']).to(DEV).load_pretrained(gmf, mlp, alpha=alpha).eval()
    users, items = np.arange(R.N_USERS), np.arange(R.N_ITEMS)
    (yg, eg), (ym, em) = R.model_bound(pg, users, items), R.model_bound(pm, users, items)
    want = alpha * yg + (1. - alpha) * ym
    # the scaled out_* vectors are rounded to float32 once more: u |w| |z| per dot product, under a quarter of the gamma(H + 1) |w| |z| that
    # the models' own bounds hold for it (H >= 3); the mixed bias and the sum cost u each
    bound = 1.25 * (alpha * eg + (1. - alpha) * em) + 3 * R.U * (alpha * yg.abs() + (1. - alpha) * ym.abs() + want.abs())
    with torch.no_grad():
        got = net.combine_user_item_representations(net.get_user_representations(torch.from_numpy(users).to(DEV)),
                                                    net.get_item_representations(torch.from_numpy(items).to(DEV)))
    ratio = float(((got.double().cpu() - want).abs() / bound).max())
    print(f'alpha {alpha}: largest error / bound {ratio:.3f}')
    assert ratio <= 1.


def test_deterministic_training_refuses_widths_off_multiples_of_4_before_any_launch():
    Sm = S()
    u, i, _ = R.batch()
    ud, idv = torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV)
    lib = _mod('_lib')
    prev = Sm.ops.set_deterministic(True)
    lib.CALL_LOG = []
    try:
        for layers in ((8, 5, 3), (6, 4), (5,)):                  # a tail width, H1 of a deeper model, H1 alone
            net = Sm.NeuMF(R.N_USERS, R.N_ITEMS, gmf_dim=4, mlp_dim=8, mlp_layers=layers).to(DEV).train()
            with pytest.raises(ValueError, match='multiples of 4'):
                net(ud, idv)
        assert [n for n, _ in lib.CALL_LOG] == []
        Sm.NeuMF(R.N_USERS, R.N_ITEMS, gmf_dim=4, mlp_dim=8, mlp_layers=(8, 5, 3)).to(DEV).eval()(ud, idv)      # evaluation is not affected
    finally:
        lib.CALL_LOG = None
        Sm.ops.set_deterministic(prev)


def test_combine_in_training_mode_sees_the_current_tail_weights():
    cfg = R.CONFIGS['full']
    net = _net(cfg, R.params(seed=8, **cfg)).train()
    users, items = torch.arange(R.N_USERS, device=DEV), torch.arange(R.N_ITEMS, device=DEV)
    with torch.no_grad():
        ur, ir = net.get_user_representations(users), net.get_item_representations(items)
        before = net.combine_user_item_representations(ur, ir)
        net.out_bias.add_(1.)
        net.mlp_tail[0].weight.mul_(0.5)
        moved = net.combine_user_item_representations(ur, ir)
        fresh = net.eval().combine_user_item_representations(ur, ir)
    _assert_bits(moved.cpu(), fresh.cpu(), 'the scores after the weights moved')
    assert not torch.equal(moved, before)
