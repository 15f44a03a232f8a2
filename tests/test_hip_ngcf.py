"""NGCF (ngcf.py) on the GPU: the model against float64 autograd with the same dropout masks, no layers as plain matrix factorisation,
the Trainer in deterministic mode, the evaluation routes against the float64 ranking, and the eval-mode cache of the propagated table.
References: tests/ngcf_ref.py."""
from importlib import import_module

import numpy as np
import pytest
import torch

import lightgcn_ref as L
import ngcf_ref as R
import scorer_truth_util as T
from hip_testutil import DEV, S, _assert_bits

pytestmark = pytest.mark.gpu
FWD, BWD = 'sbr_ngcf_layer_fwd', 'sbr_ngcf_layer_bwd'


def _mod(name):
    return import_module(S().ops.__name__.rsplit('.', 1)[0] + '.' + name)


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _loss(n_items, neg):
    return S().RecBayesianPersonalizedRankingLoss(n_items=n_items, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=neg)


def _net(g, sd, d, layer_sizes, p=0.0):
    net = S().NGCF(g.n_users, g.n_items, g.m, embedding_dim=d, layer_sizes=layer_sizes, message_dropout=p, leaky_slope=R.SLOPE)
    net.load_state_dict({k: t32(v) for k, v in sd.items()})
    return net.to(DEV)


def _drawn_seed(torch_seed):
    """the seed a training forward draws from torch's CPU generator after ``torch.manual_seed(torch_seed)``"""
    torch.manual_seed(torch_seed)
    seed = int(torch.randint(0, 1 << 62, (1,)).item())
    torch.manual_seed(torch_seed)
    return seed


# ---- 1. the model against float64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p', R.RATES)
@pytest.mark.parametrize('d', [8, 64])
@pytest.mark.parametrize('layer_sizes', [(), (8,), (64, 64, 64)], ids=['L0', 'L1', 'L3'])
def test_model_logits_loss_and_gradients_against_float64(layer_sizes, d, p):
    """Tolerance: 8 x the error of the same formula in torch float32 on the CPU against float64 on these inputs and masks
    (lightgcn_ref.yardstick, no floor), for the logits, the loss and every parameter's gradient. The masks are the restatement's, from
    the seed the model draws."""
    g, _, _, u, i, labels = L.model_world(d)
    sd = R.model_params(g, d, layer_sizes)
    n_layers = len(layer_sizes)
    masks = R.model_masks(g, layer_sizes, p, _drawn_seed(17))
    ref = R.model_torch(g, sd, u, i, labels, n_layers, R.SLOPE, masks, R.inv_keep32(p), torch.float64)
    cpu = R.model_torch(g, sd, u, i, labels, n_layers, R.SLOPE, masks, R.inv_keep32(p), torch.float32)
    net = _net(g, sd, d, layer_sizes, p).train()
    torch.manual_seed(17)
    logits = net(torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV))
    loss = _loss(30, 4).compute_loss(logits, torch.from_numpy(labels).to(DEV))
    loss.backward()
    got = {'logits': logits.detach(), 'loss': loss.detach().reshape(()), **{k: q.grad for k, q in net.named_parameters()}}
    assert sorted(k for k in got if k not in ('logits', 'loss')) == sorted(R.param_names(n_layers))
    worst = []
    for k in ['logits', 'loss'] + R.param_names(n_layers):
        e_cpu = L.yardstick(ref[k], cpu[k])
        err = float((got[k].cpu().double().reshape(ref[k].shape) - ref[k]).abs().max())
        print(f'layers={layer_sizes} D={d} p={p} {k}: error {err:.3e}, float32 on the CPU {e_cpu:.3e}, allowed {L.FACTOR * e_cpu:.3e}')
        worst.append((k, err, L.FACTOR * e_cpu))
    for k, err, tol in worst:
        assert err <= tol, f'{k}: error {err:.3e} over 8 x the float32 CPU error = {tol:.3e}'


def test_no_layers_equals_matrix_factorisation_bit_for_bit():
    g, uw, iw, u, i, labels = L.model_world(64)
    net = _net(g, {'user_embeddings.weight': uw, 'item_embeddings.weight': iw}, 64, ()).train()
    mf = S().SGDMatrixFactorization(40, 30, 64)
    mf.load_state_dict(net.state_dict())
    mf = mf.to(DEV).train()
    ud, idd = torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV)
    lib = _mod('_lib')
    lib.CALL_LOG = []
    try:
        a = net(ud, idd)
        a.sum().backward()
        net.eval()
        with torch.no_grad():
            items = torch.arange(30, device=DEV)
            sa = net.combine_user_item_representations(net.get_user_representations(ud), net.get_item_representations(items))
        names = [n for n, _ in lib.CALL_LOG]
    finally:
        lib.CALL_LOG = None
    assert FWD not in names and BWD not in names and 'sbr_graph_propagate_f32' not in names
    _assert_bits(a.detach().cpu(), mf(ud, idd).detach().cpu(), 'training logits')
    mf.eval()
    with torch.no_grad():
        sb = mf.combine_user_item_representations(mf.get_user_representations(ud), mf.get_item_representations(items))
    _assert_bits(sa.cpu(), sb.cpu(), 'all-pairs scores')


# ---- 2. the Trainer, deterministic mode --------------------------------------------------------------------------------------------------------
def _train_5(seed):
    Sm = S()
    Sm.reproducible(seed)
    ds = Sm.SyntheticDataset(300, 200, 5000, seed=1, n_negative_samples=3)
    net = Sm.ALGORITHMS['ngcf'].build_from_conf({'embedding_dim': 24, 'layer_sizes': (16, 12), 'message_dropout': 0.2}, ds)
    init = {k: v.detach().clone() for k, v in net.state_dict().items()}
    conf = {'learn': {'lr': 1e-2, 'wd': 1e-4, 'optimizer': 'adamw'}, 'run_settings': {'device': DEV}}
    tr = Sm.Trainer(net, None, None, _loss(200, 3), conf)
    net.train()
    it = iter(Sm.NegativeSamplingDataLoader(ds, batch_size=64, shuffle=True))
    before = Sm.ops.nondeterministic_launches()
    for _ in range(5):
        tr.train_step(*next(it))
    torch.cuda.synchronize()
    assert Sm.ops.nondeterministic_launches() == before
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, init


def test_five_trainer_steps_twice_give_identical_state_dicts():
    Sm = S()
    prev = Sm.ops.is_deterministic()
    try:
        (a, init), (b, _), (c, _) = _train_5(3), _train_5(3), _train_5(4)
    finally:
        Sm.ops.set_deterministic(prev)
    assert sorted(a) == sorted(R.param_names(2))
    for k in a:
        _assert_bits(a[k], b[k], k)
    assert not torch.equal(a['user_embeddings.weight'], c['user_embeddings.weight']) and not torch.equal(a['w_gc.0'], c['w_gc.0'])
    for k in ('item_embeddings.weight', 'w_gc.0', 'w_bi.1', 'b.1'):
        assert float((a[k] - init[k].cpu()).abs().max()) > 1e-3, f'the steps moved {k}'


# ---- 3. evaluation -----------------------------------------------------------------------------------------------------------------------------
class _EvalWorld:
    def __init__(self, layer_sizes):
        Sm = S()
        self.ds = Sm.SyntheticDataset(600, 500, 12000, seed=4, n_negative_samples=3, holdout_per_user=1)
        self.g = L.Graph(self.ds.user_sampling_matrix_train)
        self.L = len(layer_sizes)
        sd = R.model_params(self.g, 64, layer_sizes, seed=2)
        self.net = _net(self.g, sd, 64, layer_sizes, 0.3).eval()
        self.view = self.ds.eval_view()
        e64, bound = torch.from_numpy(R.table64(self.g, sd, self.L)), torch.from_numpy(R.table_bound(self.g, sd, self.L))
        self.u64, self.i64, bu, bi = e64[:600], e64[600:], bound[:600], bound[600:]
        excluded = torch.from_numpy(self.view.exclude_data.toarray() != 0)
        self.masked = (self.u64 @ self.i64.t()).masked_fill(excluded, -float('inf')).to(DEV)
        # the scorer's tolerance on the representations it is given, plus what the representations' own derived bound can move a score by
        self.tol = (T.C_TOL * 2.0 ** -24 * (self.u64.abs() @ self.i64.abs().t()) + bu @ self.i64.abs().t() + (self.u64.abs() + bu) @ bi.t()).to(DEV)

    def lists(self, scorer):
        Sm = S()
        ev = Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=(1, 10, 20)), dataset=self.view)
        got = []
        loader = type('L', (), {'dataset': self.view, 'batch_size': 256})()
        lib = _mod('_lib')
        lib.CALL_LOG = []
        try:
            Sm.evaluation._score_split(self.net, loader, ev, DEV, scorer, 256, False, 32, lambda s, u_, v, ix: got.append((v, ix)))
            names = [n for n, _ in lib.CALL_LOG]
        finally:
            lib.CALL_LOG = None
        return (torch.cat([g[0] for g in got]), torch.cat([g[1] for g in got])), names


@pytest.mark.parametrize('scorer,layer_sizes', [('fp32', (64, 64, 64)), ('fp32_fused', (64,))], ids=['fp32-256', 'fp32_fused-128'])
def test_evaluation_lists_against_the_float64_ranking(scorer, layer_sizes):
    """600 users in chunks of 256: the top-20 lists against the float64 ranking with the near-tie acceptance of
    tests/scorer_truth_util.py; the whole evaluation costs L forward launches, draws no mask (the model's message_dropout is 0.3) and
    does not depend on torch's seed"""
    w = _EvalWorld(layer_sizes)
    assert w.net.repr_dim == 64 * (1 + len(layer_sizes))
    torch.manual_seed(1)
    got, names = w.lists(scorer)
    assert names.count(FWD) == w.L and BWD not in names, names.count(FWD)
    assert any(n.startswith('sbr_score_topk_f32s') for n in names) == (scorer == 'fp32_fused'), set(names)
    T.check_against_truth(got, torch.arange(600, device=DEV), w.masked, w.tol, 20, what=scorer)
    w.net.train().eval()                                                                  # drops the cached table
    torch.manual_seed(2)
    again, names = w.lists(scorer)
    assert names.count(FWD) == w.L
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1]), 'the evaluation depends on the seed'


def test_the_evaluation_cache_is_rebuilt_when_the_parameters_change():
    Sm = S()
    g, _, _, u, i, labels = L.model_world(8)
    sd = R.model_params(g, 8, (8, 6))
    net = _net(g, sd, 8, (8, 6), 0.0).eval()
    ud = torch.arange(40, device=DEV)
    lib = _mod('_lib')

    def reps():
        lib.CALL_LOG = []
        try:
            with torch.no_grad():
                out = net.get_user_representations(ud).clone(), net.get_item_representations(torch.arange(30, device=DEV)).clone()
            return out, [n for n, _ in lib.CALL_LOG].count(FWD)
        finally:
            lib.CALL_LOG = None

    def want():
        cur = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
        x = np.concatenate([cur['user_embeddings.weight'], cur['item_embeddings.weight']])
        parts = [x]
        for l in range(2):
            r = R.layer32(g, x, cur[f'w_gc.{l}'], cur[f'w_bi.{l}'], cur[f'b.{l}'], R.SLOPE)
            x = r['h']
            parts.append(r['out'])
        e = np.concatenate(parts, 1)
        return t32(e[:40]), t32(e[40:])

    def step_inputs():
        return _loss(30, 4).compute_loss(net(torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV)), torch.from_numpy(labels).to(DEV))

    def check(what, prev_u=None):
        (r_u, r_i), n = reps()
        assert n == 2, f'{what}: {n} forward launches'
        if prev_u is not None:
            assert not torch.equal(r_u, prev_u), what
        _assert_bits(r_u.cpu(), want()[0], what)
        _assert_bits(r_i.cpu(), want()[1], what)
        assert reps()[1] == 0, f'{what}: a second evaluation propagates again'
        return r_u

    a_u = check('first evaluation')
    assert tuple(a_u.shape) == (40, 22)
    # a torch optimizer step on a layer weight alone (the tables keep their version counters)
    opt = torch.optim.SGD([net.w_bi[1]], lr=0.5)
    step_inputs().backward()
    opt.step()
    b_u = check('after a torch optimizer step on w_bi.1', a_u)
    opt = torch.optim.SGD(net.parameters(), lr=0.5)
    net.zero_grad()
    step_inputs().backward()
    opt.step()
    b_u = check('after a torch optimizer step', b_u)
    # the engine's optimizer writes through raw pointers: it drops the table itself on every step
    fused = Sm.FusedOptimizer(net, 'adam', 1e-1, 0.)
    (r_u, _), n = reps()
    assert n == 2 and torch.equal(r_u, b_u), 'moving the parameters into the flat buffer changes their storage, not their values'
    assert reps()[1] == 0
    fused.zero_grad()
    step_inputs().backward()
    versions = net._cache_key()
    fused.step()
    assert net._cache_key() == versions and not net.training
    c_u = check('after the fused optimizer step', b_u)
    conf = {'learn': {'lr': 1e-1, 'wd': 0., 'optimizer': 'adam'}, 'run_settings': {'device': DEV}}
    tr = Sm.Trainer(net, None, None, _loss(30, 4), conf)
    net.train()
    tr.train_step(torch.from_numpy(u), torch.from_numpy(i), torch.from_numpy(labels))
    net.eval()
    check('after the Trainer step', c_u)
    net.load_state_dict({k: t32(v) for k, v in sd.items()})
    d_u = check('after load_state_dict')
    _assert_bits(d_u.cpu(), a_u.cpu(), 'after load_state_dict')
    assert net.get_user_representations(ud).requires_grad
