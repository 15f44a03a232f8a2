"""DirectAU (directau.py) on the GPU: one training step's loss terms and table gradients against the float64 restatement of
tests/directau_ref.py, the Trainer on the autograd path with ``rec_loss = align``, bit-identical repeated trainings, the evaluation routes
against the raw dot product of the encoder rows, checkpoints, the autograd fall-back of a SingleBranchNet Trainer given ``align``, and
``gamma = 0`` as matrix factorisation trained on alignment alone."""
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import directau_ref as R
import scorer_truth_util as T
from hip_testutil import DEV, S, _assert_bits

pytestmark = pytest.mark.gpu
D = 16


def _mod(name):
    return import_module(S().ops.__name__.rsplit('.', 1)[0] + '.' + name)


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _align(n_items=40, neg=3):
    return S().RecAlignmentLoss(n_items=n_items, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=neg)


def _net(m, uw, iw, n_layers, gamma=1.0, t=2.0):
    net = S().DirectAU(uw.shape[0], iw.shape[0], embedding_dim=uw.shape[1], gamma=gamma, t=t, n_layers=n_layers,
                       train_matrix=m if n_layers else None)
    net.load_state_dict({'user_embeddings.weight': t32(uw), 'item_embeddings.weight': t32(iw)})
    return net.to(DEV)


def _step(net, u, i, labels):
    logits = net(torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV))
    rec = _align().compute_loss(logits, torch.from_numpy(labels).to(DEV))
    other = net.get_and_reset_other_loss()
    (rec + other['reg_loss']).backward()
    return logits.detach(), rec.detach(), other


@pytest.mark.parametrize('n_layers', [0, 2])
def test_one_training_step_against_float64(n_layers):
    """Loss terms: the uniformity bound pushed through the normalisation's Jacobian (directau_ref.model_loss_bound), with the propagated
    rows' own derived bound as the input error for n_layers = 2; the alignment is a float64 sum of fp32 cosines, each off by at most two
    normalisation errors and a dot product's (D + 2) u. Table gradients: 8 x the error of the same step in torch float32 on the CPU."""
    gamma, t = 0.7, 2.0
    m, uw, iw, u, i, labels = R.model_world(D)
    ref = R.step_torch(m, uw, iw, u, i, labels, n_layers, gamma, t, torch.float64)
    cpu = R.step_torch(m, uw, iw, u, i, labels, n_layers, gamma, t, torch.float32)
    net = _net(m, uw, iw, n_layers, gamma, t).train()
    logits, rec, other = _step(net, u, i, labels)
    rel_in = 0.0
    if n_layers:
        e0 = np.concatenate([uw, iw]).astype(np.float64)
        a = R.a_hat(m)
        e64 = (e0 + a @ e0 + a @ (a @ e0)) / 3
        used = np.concatenate([u, 50 + i.reshape(-1)])
        rel_in = float((np.linalg.norm(R.mean_bound(m, e0, 2)[used], axis=1) / np.linalg.norm(e64[used], axis=1)).max())
    delta = R.hat_error(D, rel_in)
    b_logit = R.SECOND * (2 * delta + (D + 2) * R.U)
    figures = [('logits', float((logits.cpu().double() - ref['logits']).abs().max()), b_logit),
               ('align', abs(float(rec) - float(ref['align'])), 2 * b_logit),
               ('uniform_u', abs(float(other['uniform_u']) - float(ref['uniform_u'])), R.model_loss_bound(ref['u_hat'].numpy(), t, D, rel_in)),
               ('uniform_i', abs(float(other['uniform_i']) - float(ref['uniform_i'])),
                R.model_loss_bound(ref['i_hat'][:, 0].numpy(), t, D, rel_in))]
    figures.append(('reg_loss', abs(float(other['reg_loss'].detach()) - float(ref['reg'])), gamma * (figures[2][2] + figures[3][2]) / 2 + 4 * R.U * abs(float(ref['reg']))))
    for k, p in net.named_parameters():
        figures.append((k, float((p.grad.cpu().double() - ref[k]).abs().max()), R.FACTOR * R.yardstick(ref[k], cpu[k])))
    for k, err, tol in figures:
        print(f'L={n_layers} {k}: error {err:.3e}, allowed {tol:.3e}')
    for k, err, tol in figures:
        assert err <= tol, f'{k}: error {err:.3e} over {tol:.3e}'
    assert float(net.user_embeddings.weight.grad.abs().max()) > 0 and rec.dtype == torch.float64
    with pytest.raises(S().SibrarHipError, match='sbr_uniformity_fwd'):          # a batch of one row: the kernel's refusal surfaces
        net(torch.from_numpy(u[:1]).to(DEV), torch.from_numpy(i[:1]).to(DEV))
    net.get_and_reset_other_loss()


def test_gamma_zero_is_matrix_factorisation_trained_on_alignment_alone():
    prev = S().ops.set_deterministic(True)         # the lookups' gradient adds repeated rows: only its fixed-order form has bits to compare
    try:
        _gamma_zero()
    finally:
        S().ops.set_deterministic(prev)


def _gamma_zero():
    m, uw, iw, u, i, labels = R.model_world(D)
    net = _net(m, uw, iw, 0, gamma=0.0).train()
    mf = S().SGDMatrixFactorization(50, 40, D)
    mf.load_state_dict(net.state_dict())
    mf = mf.to(DEV).train()
    ud, idd = torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV)
    _assert_bits(net.get_user_representations(ud).detach().cpu(), mf.get_user_representations(ud).detach().cpu(), 'user lookups')
    _assert_bits(net.get_item_representations(idd).detach().cpu(), mf.get_item_representations(idd).detach().cpu(), 'item lookups')
    logits, rec, other = _step(net, u, i, labels)
    assert float(other['reg_loss']) == 0.0 and float(other['uniform_u']) < 0 and float(other['uniform_i']) < 0
    # align alone, by the package's own ops on mf's lookups
    ops = S().ops
    uh = ops.L2NormalizeFn.apply(mf.get_user_representations(ud))
    ir = mf.get_item_representations(idd)
    ih = ops.L2NormalizeFn.apply(ir.reshape(-1, D)).view(ir.shape)
    z = mf.combine_user_item_representations(uh, ih)
    _assert_bits(logits.cpu(), z.detach().cpu(), 'cosine logits')
    _align().compute_loss(z, torch.from_numpy(labels).to(DEV)).backward()
    for (k, p), (_, q) in zip(net.named_parameters(), mf.named_parameters()):
        _assert_bits(p.grad.cpu(), q.grad.cpu(), f'{k}: gradient of align alone')
    net.eval(), mf.eval()
    with torch.no_grad():
        _assert_bits(net(ud, idd).cpu(), mf(ud, idd).cpu(), 'evaluation scores are raw dot products')


def _dataset():
    return S().SyntheticDataset(50, 40, 700, seed=1, n_negative_samples=3)


def _trainer(net, loss, ds, lr=1e-2):
    Sm = S()
    loader = Sm.NegativeSamplingDataLoader(ds, batch_size=37, shuffle=True)
    whole = len(loader.rows) // 37                                             # the trailing batch may hold one row, which the kernel refuses
    conf = {'learn': {'lr': lr, 'wd': 0., 'optimizer': 'adam', 'max_batches_per_epoch': whole}, 'run_settings': {'device': DEV}}
    return Sm.Trainer(net, loader, None, loss, conf)


def _train_two_epochs(seed, n_layers=2):
    Sm = S()
    Sm.reproducible(seed)
    ds = _dataset()
    net = Sm.ALGORITHMS['directau'].build_from_conf({'embedding_dim': D, 'gamma': 1.0, 't': 2.0, 'n_layers': n_layers}, ds)
    tr = _trainer(net, _align(), ds)
    assert tr.fused is None
    before = Sm.ops.nondeterministic_launches()
    epochs = [tr.train(), tr.train()]
    torch.cuda.synchronize()
    assert Sm.ops.nondeterministic_launches() == before
    return epochs, {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def test_trainer_two_epochs_decrease_and_repeat_bit_for_bit():
    Sm = S()
    prev = Sm.ops.is_deterministic()
    try:
        (e0, e1), a = _train_two_epochs(3)
        _, b = _train_two_epochs(3)
        _, c = _train_two_epochs(4)
    finally:
        Sm.ops.set_deterministic(prev)
    for ep in (e0, e1):
        assert {'train/loss', 'train/rec_loss', 'train/reg_loss', 'train/uniform_u', 'train/uniform_i'} <= set(ep), set(ep)
        assert all(np.isfinite(v) for v in ep.values())
    print(f'epoch 0 {e0}\nepoch 1 {e1}')
    assert e1['train/loss'] < e0['train/loss']
    assert abs(e0['train/loss'] - (e0['train/rec_loss'] + e0['train/reg_loss'])) <= 1e-6 * abs(e0['train/loss']) + 1e-9
    assert abs(e0['train/reg_loss'] - (e0['train/uniform_u'] + e0['train/uniform_i']) / 2) <= 1e-5
    for k in a:
        _assert_bits(a[k], b[k], k)
    assert not torch.equal(a['user_embeddings.weight'], c['user_embeddings.weight'])


class _EvalWorld:
    def __init__(self):
        Sm = S()
        self.ds = Sm.SyntheticDataset(600, 500, 12000, seed=4, n_negative_samples=3, holdout_per_user=1)
        gen = torch.Generator().manual_seed(12)
        self.uw, self.iw = torch.randn(600, 64, generator=gen) * 0.5, torch.randn(500, 64, generator=gen) * 0.5
        self.net = _net(None, self.uw.numpy(), self.iw.numpy(), 0).eval()
        self.view = self.ds.eval_view()
        u64, i64 = self.uw.double(), self.iw.double()
        excluded = torch.from_numpy(self.view.exclude_data.toarray() != 0)
        self.masked = (u64 @ i64.t()).masked_fill(excluded, -float('inf')).to(DEV)      # the RAW dot product: no normalisation in eval()
        self.tol = (T.C_TOL * 2.0 ** -24 * (u64.abs() @ i64.abs().t())).to(DEV)

    def lists(self, scorer):
        Sm = S()
        ev = Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=(1, 10, 20)), dataset=self.view)
        got = []
        loader = type('L', (), {'dataset': self.view, 'batch_size': 256})()
        L = _mod('_lib')
        L.CALL_LOG = []
        try:
            Sm.evaluation._score_split(self.net, loader, ev, DEV, scorer, 256, False, 32, lambda s, u_, v, ix: got.append((v, ix)))
            names = [n for n, _ in L.CALL_LOG]
        finally:
            L.CALL_LOG = None
        return (torch.cat([g[0] for g in got]), torch.cat([g[1] for g in got])), names


@pytest.fixture(scope='module')
def eval_world():
    return _EvalWorld()


@pytest.mark.parametrize('scorer', ['fp32', 'fp32_fused', 'fp16_fused'])
def test_evaluation_ranks_by_the_raw_dot_product(eval_world, scorer):
    """embedding_dim 64: every route the model qualifies for. The fp32 routes against the float64 ranking of the raw dot product with the
    near-tie acceptance of tests/scorer_truth_util.py; the fp16 route is held to its metrics only (its lists follow fp16-rounded rows)."""
    w = eval_world
    Sm = S()
    if scorer != 'fp16_fused':
        got, names = w.lists(scorer)
        assert any(n.startswith('sbr_score_topk_f32s') for n in names) == (scorer == 'fp32_fused'), set(names)
        assert 'sbr_l2norm_fwd' not in names and 'sbr_uniformity_fwd' not in names
        T.check_against_truth(got, torch.arange(600, device=DEV), w.masked, w.tol, 20, what=scorer)
    res = Sm.evaluate_recommender_algorithm(w.net, type('L', (), {'dataset': w.view, 'batch_size': 256})(),
                                            Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=(10,)), dataset=w.view), DEV, scorer=scorer)
    assert 0.0 <= res['ndcg@10'] <= 1.0


def test_checkpoints(tmp_path):
    Sm = S()
    m, uw, iw, u, i, labels = R.model_world(D)
    mf = Sm.SGDMatrixFactorization(50, 40, D)
    net = Sm.DirectAU(50, 40, embedding_dim=D)
    net.load_state_dict(mf.state_dict())
    assert torch.equal(net.item_embeddings.weight, mf.item_embeddings.weight)
    lg = Sm.LightGCN(50, 40, m, embedding_dim=D, n_layers=2)
    net2 = Sm.DirectAU(50, 40, embedding_dim=D, n_layers=2, train_matrix=m)
    net2.load_state_dict(lg.state_dict())
    assert torch.equal(net2.user_embeddings.weight, lg.user_embeddings.weight)
    net2 = net2.to(DEV)
    net2.save_model_to_path(str(tmp_path))
    assert os.path.exists(os.path.join(str(tmp_path), 'model.pth'))
    back = Sm.DirectAU(50, 40, embedding_dim=D, n_layers=2, train_matrix=m).to(DEV)
    back.load_model_from_path(str(tmp_path))
    for k, v in net2.state_dict().items():
        _assert_bits(back.state_dict()[k].cpu(), v.cpu(), k)
    ud, idd = torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV)
    net2.eval(), back.eval()
    with torch.no_grad():
        _assert_bits(back(ud, idd).cpu(), net2(ud, idd).cpu(), 'scores after the round trip')


def test_a_single_branch_net_trainer_given_align_takes_the_autograd_step():
    Sm = S()
    torch.manual_seed(0)
    ds = Sm.SyntheticDataset(300, 200, 4000, item_dense={'text': 32}, item_tags={'genres': (9, 3)}, seed=3, n_negative_samples=3)
    cfg = {'shared_common_dim': 16, 'user': {'feature_name': 'user_embedding', 'embedding_dim': -1},
           'item': {'features': [{'feature_name': 'interactions'}, {'feature_name': 'genres'}, {'feature_name': 'text'}],
                    'single_branch_hidden_layers': [16], 'preference_hidden_layers': [], 'common_modality_dim': 16,
                    'embedding_regularization_type': 'pairwise_single', 'regularization_weight': 0.1}}
    net = Sm.SingleBranchNet(Sm.SingleBranchNetConfig.from_dict(cfg), ds)
    conf = {'learn': {'lr': 1e-3, 'wd': 0., 'optimizer': 'adam'}, 'run_settings': {'device': DEV}}
    tr = Sm.Trainer(net, None, None, _align(200, 3), conf)
    assert tr.fused is None, 'no fused step for a loss without a fused kernel'
    with pytest.raises(NotImplementedError):
        Sm.FusedTrainStep(net, _align(200, 3), tr.optimizer)
    net.train()
    before = net.item_embedding_module.state_dict()
    before = {k: v.detach().clone() for k, v in before.items()}
    total, rec, regs = tr.train_step(*next(iter(Sm.NegativeSamplingDataLoader(ds, batch_size=32))))
    assert np.isfinite(float(total)) and rec.dtype == torch.float64 and 'reg_loss' in regs
    assert any(not torch.equal(v, before[k]) for k, v in net.item_embedding_module.state_dict().items()), 'the step moved the parameters'
