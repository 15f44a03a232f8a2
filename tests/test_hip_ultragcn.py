"""UltraGCN (ultragcn.py) on the GPU: three Adam steps on the planted world against the float64 model of tests/ultragcn_ref.py within 8 times
the error of the same network in torch float32 on the CPU; bit-identical repeated trainings in deterministic mode with the counter of
arrival-order launches at rest; the Trainer with ``rec_loss: none``; an ``mf`` checkpoint; the evaluation routes at embedding_dim 64; and
30 epochs on the planted world against PopularItems. Measured on an MI355X: user table error 3.12e-08 against 4.50e-08 for float32 on the
CPU, item table 2.06e-08 against 2.06e-08; NDCG@10 0.610 against 0.071 for PopularItems. Reached entries: 'sbr_cooc_weight_topk', 'sbr_ultragcn_loss_fwd_bwd',
'sbr_scatter_add_scaled_rows_sorted'."""
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import scorer_truth_util as T
import ultragcn_ref as R
from hip_testutil import DEV, S, _assert_bits

pytestmark = pytest.mark.gpu
D, K, N, LR = 16, 6, 12, 1e-2
SC = (1e-3, 1.0, 1e-3, 1.0, 20.0, 0.5)


def _mod(name):
    return import_module(S().ops.__name__.rsplit('.', 1)[0] + '.' + name)


def _tables(seed=0, d=D, std=0.1):
    g = torch.Generator().manual_seed(100 + seed)
    return (torch.randn(60, d, generator=g) * std).numpy(), (torch.randn(40, d, generator=g) * std).numpy()


def _net(m, uw, iw, k=K, sc=SC):
    net = S().UltraGCN(60, 40, m, embedding_dim=uw.shape[1], n_neighbors=k, w1=sc[0], w2=sc[1], w3=sc[2], w4=sc[3], negative_weight=sc[4], lam=sc[5])
    net.load_state_dict({'user_embeddings.weight': torch.from_numpy(uw), 'item_embeddings.weight': torch.from_numpy(iw)})
    return net.to(DEV)


def _train(net, batches, lr=LR):
    Sm = S()
    net.train()
    opt = Sm.FusedOptimizer(net, 'adam', lr, 0.)
    losses = []
    for u, i in batches:
        scores = net(torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV))
        assert scores.shape == i.shape and not scores.requires_grad
        other = net.get_and_reset_other_loss()
        (Sm.RecNoLoss(n_items=40).compute_loss(scores, None) + other['reg_loss']).backward()
        opt.step()
        opt.zero_grad()
        losses.append((float(other['reg_loss']), float(other['pos_loss']), float(other['neg_loss']), float(other['nbr_loss'])))
    torch.cuda.synchronize()
    return net.user_embeddings.weight.detach().cpu(), net.item_embeddings.weight.detach().cpu(), losses


def test_three_adam_steps_against_the_float64_model():
    m = R.planted_world()
    uw, iw = _tables()
    batches = R.planted_batches(m, 3, 48, N)
    ref = R.train_torch(m, uw, iw, batches, K, SC, LR, torch.float64)
    cpu = R.train_torch(m, uw, iw, batches, K, SC, LR, torch.float32)
    net = _net(m, uw, iw)
    got = _train(net, batches)
    # the lists and scales the model built are the restatement's
    bu, bi, row, col = R.scales32(m)
    want = R.lists32(m, row, col, K)
    for g, w, name in zip((net.nbr_idx, net.nbr_val, net.nbr_len), want, ('nbr_idx', 'nbr_val', 'nbr_len')):
        assert np.array_equal(g.cpu().numpy().view(np.int32), w.view(np.int32)), name
    assert net._matrix is None, 'the matrix is dropped once the lists are built'
    for k, (g, r, c) in enumerate(zip(got[:2], ref[:2], cpu[:2])):
        err, yard = float((g.double() - r).abs().max()), float((c.double() - r).abs().max())
        print(f'{("user", "item")[k]} table after 3 Adam steps: error {err:.3e}, float32 on the CPU {yard:.3e}, allowed {R.FACTOR * yard:.3e}')
        assert err <= R.FACTOR * yard
        assert float((g.double() - torch.from_numpy((uw, iw)[k]).double()).abs().max()) > 0.5 * LR, 'the tables moved'
    for step, (g, r, c) in enumerate(zip(got[2], ref[2], cpu[2])):
        yard = abs(c - r)
        print(f'step {step}: loss {g[0]:.6f} (float64 {r:.6f}), error {abs(g[0] - r):.3e}, float32 on the CPU {yard:.3e}')
        assert abs(g[0] - r) <= R.FACTOR * yard + 2 * R.U * abs(r), 'the loss is a float32 scalar: two roundings of its own'
        assert abs(g[0] - (g[1] + SC[4] * g[2] + SC[5] * g[3])) <= 4 * R.U * abs(g[0]) and min(g[1:]) > 0


def test_deterministic_mode_repeats_bit_for_bit():
    Sm = S()
    m = R.planted_world()
    uw, iw = _tables(1)
    batches = R.planted_batches(m, 4, 48, N, seed=1)
    prev = Sm.ops.set_deterministic(True)
    try:
        before = Sm.ops.nondeterministic_launches()
        a = _train(_net(m, uw, iw), batches)
        b = _train(_net(m, uw, iw), batches)
        assert Sm.ops.nondeterministic_launches() == before, 'a training step took an arrival-order path'
    finally:
        Sm.ops.set_deterministic(prev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    assert not torch.equal(a[0], torch.from_numpy(uw))


def test_trainer_reports_the_parts_and_an_mf_checkpoint_loads(tmp_path):
    Sm = S()
    prev = Sm.ops.is_deterministic()
    Sm.reproducible(5)
    try:
        ds = Sm.SyntheticDataset(50, 40, 700, seed=1, n_negative_samples=7)
        net = Sm.ALGORITHMS['ultragcn'].build_from_conf({'embedding_dim': D, 'n_neighbors': K, 'init_std': 0.05, 'negative_weight': 20., 'lam': 0.1}, ds)
        loss = Sm.RecommenderSystemLoss.build_from_conf({'learn': {'rec_loss': 'none'}, 'dataset': {'n_negative_samples': 7}}, ds)
        loader = Sm.NegativeSamplingDataLoader(ds, batch_size=64, shuffle=True)
        conf = {'learn': {'lr': 1e-2, 'wd': 0., 'optimizer': 'adam'}, 'run_settings': {'device': DEV}}
        tr = Sm.Trainer(net, loader, None, loss, conf)
        assert tr.fused is None
        e0, e1 = tr.train(), tr.train()
    finally:
        Sm.ops.set_deterministic(prev)
    keys = {'train/loss', 'train/rec_loss', 'train/reg_loss', 'train/pos_loss', 'train/neg_loss', 'train/nbr_loss'}
    assert keys <= set(e0), set(e0)
    print(f'epoch 0 {e0}\nepoch 1 {e1}')
    assert all(np.isfinite(v) for v in e0.values()) and e0['train/rec_loss'] == 0.0 and e0['train/loss'] == e0['train/reg_loss'] > 0
    assert abs(e0['train/reg_loss'] - (e0['train/pos_loss'] + 20. * e0['train/neg_loss'] + 0.1 * e0['train/nbr_loss'])) <= 1e-5 * e0['train/reg_loss']
    assert e1['train/loss'] < e0['train/loss']
    mf = Sm.SGDMatrixFactorization(50, 40, D)
    net.load_state_dict(mf.state_dict())
    assert torch.equal(net.item_embeddings.weight.cpu(), mf.item_embeddings.weight)
    net.save_model_to_path(str(tmp_path))
    back = Sm.UltraGCN(50, 40, ds.user_sampling_matrix_train, embedding_dim=D).to(DEV)
    back.load_model_from_path(str(tmp_path))
    for k, v in net.state_dict().items():
        _assert_bits(back.state_dict()[k].cpu(), v.cpu(), k)


@pytest.fixture(scope='module')
def eval_world():
    Sm = S()
    ds = Sm.SyntheticDataset(600, 500, 12000, seed=4, n_negative_samples=3, holdout_per_user=1)
    gen = torch.Generator().manual_seed(12)
    uw, iw = torch.randn(600, 64, generator=gen) * 0.5, torch.randn(500, 64, generator=gen) * 0.5
    net = Sm.UltraGCN(600, 500, ds.user_sampling_matrix_train, embedding_dim=64)
    net.load_state_dict({'user_embeddings.weight': uw, 'item_embeddings.weight': iw})
    view = ds.eval_view()
    u64, i64 = uw.double(), iw.double()
    excluded = torch.from_numpy(view.exclude_data.toarray() != 0)
    return SimpleNamespace(net=net.to(DEV).eval(), view=view, masked=(u64 @ i64.t()).masked_fill(excluded, -float('inf')).to(DEV),
                           tol=(T.C_TOL * 2.0 ** -24 * (u64.abs() @ i64.abs().t())).to(DEV))


@pytest.mark.parametrize('scorer', ['fp32', 'fp32_fused'])
def test_evaluation_is_matrix_factorisation_on_either_route(eval_world, scorer):
    """embedding_dim 64: the fp32_fused route is taken, and both routes give the float64 ranking of the dot product up to near-ties (the
    criterion of tests/scorer_truth_util.py, as in the other models' scorer tests)"""
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
    assert 'sbr_ultragcn_loss_fwd_bwd' not in names and 'sbr_cooc_weight_topk' not in names, 'evaluation needs neither the loss nor the lists'
    T.check_against_truth((torch.cat([g[0] for g in got]), torch.cat([g[1] for g in got])), torch.arange(600, device=DEV), w.masked, w.tol, 20,
                          what=scorer)


def test_thirty_epochs_on_the_planted_world_beat_popularity():
    Sm = S()
    train, held = R.planted_split()
    view = SimpleNamespace(n_users=60, n_items=40, items_in_split=np.arange(40), users_in_split=np.arange(60), n_items_in_split=40,
                           n_users_in_split=60, exclude_data=train.astype(bool), user_features={}, item_features={},
                           user_sampling_matrix=sp.csr_matrix((np.ones(60), (np.arange(60), held[:, 0])), shape=train.shape))

    def ndcg(alg):
        ev = Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=(10,)), dataset=view)
        return Sm.evaluate_recommender_algorithm(alg, type('L', (), {'dataset': view, 'batch_size': 64})(), ev, DEV)['ndcg@10']

    uw, iw = _tables(2)
    net = _net(train, uw, iw)
    per_epoch = -(-train.nnz // 64)
    _, _, losses = _train(net, R.planted_batches(train, 30 * per_epoch, 64, N, seed=2), lr=2e-2)
    got = ndcg(net.eval())
    pop = ndcg(Sm.PopularItems.build_from_conf({}, SimpleNamespace(user_sampling_matrix=train)))
    print(f'UltraGCN after 30 epochs: NDCG@10 {got:.4f}, PopularItems {pop:.4f}; loss {losses[0][0]:.4f} -> {losses[-1][0]:.4f}')
    assert losses[-1][0] < losses[0][0] and got > pop
