"""SimGCL / XSimGCL on the GPU (simgcl.py, ``ops.NoisyPropagateFn``): both networks against float64 autograd with the same Philox noise
injected (tests/simgcl_ref.py), the layer stack against its fp32 restatement and its backward pass against the stated Horner composition
of 'sbr_graph_propagate_f32' bit for bit, the contrast over distinct rows, cl_weight = 0, the Trainer in deterministic mode, the
evaluation table (the clean mean of the layers 1 .. L), checkpoints and the registry."""
from importlib import import_module

import numpy as np
import pytest
import torch

import lightgcn_ref as L
import scorer_truth_util as T
import simgcl_ref as R
from hip_testutil import DEV, S, _assert_bits

pytestmark = pytest.mark.gpu
NOISY, CLEAN = 'sbr_graph_propagate_noise_f32', 'sbr_graph_propagate_f32'
# A contrast term as a figure (the tests of the distinct rows): its logits are dot products of unit rows over 1 / tau = 5, so fp32 moves
# one by at most about (D + 2) * 2^-24 * 5 < 2.1e-5 at D = 64 and the mean of log-sum-exps by no more; the terms are of the order
# log N > 1. A wrong N (rows counted twice) moves a term by more than 1e-2.
CL_RTOL = 1e-4


def _mod(name):
    return import_module(S().ops.__name__.rsplit('.', 1)[0] + '.' + name)


_CSR = {}


def dev_csr(g):
    if id(g) not in _CSR:
        _CSR[id(g)] = (g, _mod('features').DeviceCSR(g.m).to(DEV))
    return _CSR[id(g)][1]


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _loss(n_items, neg):
    return S().RecBayesianPersonalizedRankingLoss(n_items=n_items, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=neg)


def _net(kind, g, uw, iw, n_layers, keep_layer=None, **kw):
    if kind == 'xsimgcl':
        kw['keep_layer'] = keep_layer
    net = S().ALGORITHMS[kind](g.n_users, g.n_items, g.m, embedding_dim=uw.shape[1], n_layers=n_layers, **kw)
    net.load_state_dict({'user_embeddings.weight': t32(uw), 'item_embeddings.weight': t32(iw)})
    return net.to(DEV)


def _logged(fn):
    lib = _mod('_lib')
    lib.CALL_LOG = []
    try:
        return fn(), list(lib.CALL_LOG)
    finally:
        lib.CALL_LOG = None


# ---- 1. both networks against float64 ------------------------------------------------------------------------------------------------------
CASES = [('simgcl', 1, None), ('simgcl', 3, None), ('xsimgcl', 1, 1), ('xsimgcl', 3, 1), ('xsimgcl', 3, 3)]


@pytest.mark.parametrize('d', [8, 64])
@pytest.mark.parametrize('kind,n_layers,keep', CASES)
def test_model_against_float64(kind, n_layers, keep, d):
    """Tolerance: 8 x the error of the same formula in torch float32 on the CPU against float64 on these inputs
    (lightgcn_ref.yardstick: the maximum absolute error of the quantity as measured, no floor), for the logits, reg_loss, the total
    loss and both table gradients alike, as tests/test_hip_lightgcn.py does. The noise is the same in all three: Philox at step 0."""
    g, uw, iw, u, i, labels = L.model_world(d)
    kw = dict(eps=0.1, cl_weight=0.2, tau=0.2, seed=5)
    ref = R.model_torch(kind, g, uw, iw, u, i, labels, n_layers, torch.float64, step=0, keep_layer=keep, **kw)
    cpu = R.model_torch(kind, g, uw, iw, u, i, labels, n_layers, torch.float32, step=0, keep_layer=keep, **kw)
    net = _net(kind, g, uw, iw, n_layers, keep, **kw).train()
    logits = net(torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV))
    rec = _loss(30, 4).compute_loss(logits, torch.from_numpy(labels).to(DEV))
    other = net.get_and_reset_other_loss()
    loss = rec + other['reg_loss']
    loss.backward()
    assert net.step == 1 and set(other) == {'reg_loss', 'cl_u', 'cl_i'} and not other['cl_u'].requires_grad
    got = {'logits': logits.detach(), 'reg_loss': other['reg_loss'].detach().reshape(()), 'loss': loss.detach().reshape(()),
           'cl_u': other['cl_u'], 'cl_i': other['cl_i'], **{k: p.grad for k, p in net.named_parameters()}}
    worst = []
    for k in ('logits', 'reg_loss', 'loss', 'user_embeddings.weight', 'item_embeddings.weight'):
        e_cpu = L.yardstick(ref[k], cpu[k])
        err = float((got[k].cpu().double().reshape(ref[k].shape) - ref[k]).abs().max())
        print(f'{kind} L={n_layers} keep={keep} D={d} {k}: error {err:.3e}, float32 on the CPU {e_cpu:.3e}, allowed {L.FACTOR * e_cpu:.3e}')
        worst.append((k, err, L.FACTOR * e_cpu))
    for k, err, tol in worst:
        assert err <= tol, f'{k}: error {err:.3e} over 8 x the float32 CPU error = {tol:.3e}'


# ---- 2. the layer stack and its backward pass, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize('n_layers,keep', [(1, 1), (3, 1), (3, 3), (3, None), (2, 2)])
def test_forward_restatement_and_horner_backward_bit_for_bit(n_layers, keep):
    g = L.world(257, 64)
    ops = S().ops
    csr = dev_csr(g)
    d, eps, seed, step, view = 12, 0.1, 9, 3, 1
    e0 = t32(L.table(g.n, d, 5)).to(DEV).requires_grad_()
    w1, w2 = t32(L.table(g.n, d, 6)).to(DEV), t32(L.table(g.n, d, 7)).to(DEV)
    before = ops.nondeterministic_launches()
    (mean, kept), log = _logged(lambda: ops.NoisyPropagateFn.apply(csr, e0, n_layers, eps, seed, step, view, keep))
    assert [n for n, _ in log] == [NOISY] * n_layers
    assert [a[-2] for _, a in log] == [R.stream_id(step, view, k) for k in range(1, n_layers + 1)]
    m_ref, k_ref = R.mean32(g, e0.detach().cpu().numpy(), n_layers, eps, seed, step, view, keep)
    _assert_bits(mean.detach().cpu(), t32(m_ref), 'the mean against the restatement')
    assert (kept is None) == (keep is None)
    loss = (mean * w1).sum()
    if keep is not None:
        _assert_bits(kept.detach().cpu(), t32(k_ref), 'the kept layer against the restatement')
        loss = loss + (kept * w2).sum()
    _, log = _logged(loss.backward)
    assert [n for n, _ in log if n.startswith('sbr_graph')] == [CLEAN] * n_layers, 'L launches of the existing entry, no other kernel'
    # the stated composition, by hand on the existing entry
    gm = w1 * (1.0 / n_layers)

    def c(k):
        return gm + w2 if k == keep else gm.clone()

    t = c(n_layers)
    for k in range(n_layers, 1, -1):
        s = c(k - 1)
        ops.graph_propagate(csr, t, sum=s, sum_scale=1.0)
        t = s
    want = ops.graph_propagate(csr, t)
    _assert_bits(e0.grad.cpu(), want.cpu(), 'gradient against the Horner composition')
    assert ops.nondeterministic_launches() == before
    # only the kept layer used: c_k is g_kept at the kept layer and zero elsewhere
    if keep is not None:
        e1 = e0.detach().clone().requires_grad_()
        (ops.NoisyPropagateFn.apply(csr, e1, n_layers, eps, seed, step, view, keep)[1] * w2).sum().backward()
        t = w2.clone() if keep == n_layers else torch.zeros_like(w2)
        for k in range(n_layers, 1, -1):
            s = w2.clone() if k - 1 == keep else torch.zeros_like(w2)
            ops.graph_propagate(csr, t, sum=s, sum_scale=1.0)
            t = s
        _assert_bits(e1.grad.cpu(), ops.graph_propagate(csr, t).cpu(), 'gradient of the kept layer alone')
    # eps = 0 takes the existing entry and gives the clean mean
    (clean, _), log = _logged(lambda: ops.NoisyPropagateFn.apply(csr, e0.detach(), n_layers, 0.0, seed, step, view, None))
    assert [n for n, _ in log] == [CLEAN] * n_layers
    _assert_bits(clean.cpu(), t32(R.mean32(g, e0.detach().cpu().numpy(), n_layers, 0.0, seed, step, view)[0]), 'the clean mean')
    for bad in (dict(n_layers=0), dict(keep=n_layers + 1), dict(keep=0), dict(view=4), dict(n_layers=64), dict(eps=-1.0)):
        a = dict(n_layers=n_layers, eps=eps, view=view, keep=keep)
        a.update(bad)
        with pytest.raises(ValueError):
            ops.NoisyPropagateFn.apply(csr, e0.detach(), a['n_layers'], a['eps'], seed, step, a['view'], a['keep'])


# ---- 3. the contrast: cl_weight = 0, distinct rows -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['simgcl', 'xsimgcl'])
def test_cl_weight_zero_leaves_the_contrast_out_of_the_gradient(kind):
    g, uw, iw, u, i, labels = L.model_world(8)
    ud, idd, ld = torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV), torch.from_numpy(labels).to(DEV)
    grads, terms = [], []
    prev = S().ops.is_deterministic()
    S().ops.set_deterministic(True)                                                       # fixed-order scatter-adds: runs compare bit for bit
    try:
        for cl_weight, add_reg in ((0.0, True), (0.2, False), (0.2, True)):
            net = _net(kind, g, uw, iw, 2, 1, cl_weight=cl_weight, seed=3).train()
            rec = _loss(30, 4).compute_loss(net(ud, idd), ld)
            other = net.get_and_reset_other_loss()
            assert other['reg_loss'].requires_grad == (cl_weight > 0)
            (rec + other['reg_loss'] if add_reg else rec).backward()
            grads.append({k: p.grad.cpu() for k, p in net.named_parameters()})
            terms.append((float(other['reg_loss'].detach()), float(other['cl_u']), float(other['cl_i'])))
    finally:
        S().ops.set_deterministic(prev)
    for k in grads[0]:
        _assert_bits(grads[0][k], grads[1][k], f'{k}: cl_weight = 0 against the recommendation loss alone')
        assert not torch.equal(grads[0][k], grads[2][k]), f'{k}: the contrast has a gradient when it is weighted'
    assert terms[0][0] == 0.0 and terms[0][1:] == terms[2][1:] and terms[0][1] > 0 and terms[0][2] > 0, 'the terms are still figures'
    assert abs(terms[2][0] - 0.2 * (terms[2][1] + terms[2][2])) <= 1e-6
    zero = _net(kind, g, uw, iw, 2, 1).get_and_reset_other_loss()
    assert all(float(v) == 0 for v in zero.values()) and set(zero) == {'reg_loss', 'cl_u', 'cl_i'}


@pytest.mark.parametrize('kind', ['simgcl', 'xsimgcl'])
def test_the_contrast_runs_over_the_distinct_rows(kind):
    g, uw, iw, u, i, labels = L.model_world(8)
    u, i = u.copy(), i.copy()
    u[10:16] = u[0]                                                                       # repeated users and repeated positives
    i[4:12, 0] = i[0, 0]
    n_u, n_i = len(np.unique(u)), len(np.unique(i[:, 0]))
    assert n_u < len(u) - 5 and n_i < len(u) - 6
    net = _net(kind, g, uw, iw, 2, 2, seed=1).train()
    _, log = _logged(lambda: net(torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV)))
    sizes = [a[4] for n, a in log if n.startswith('sbr_infonce') and n.endswith('_fwd')]
    assert sizes == [n_u, n_i], (sizes, n_u, n_i)
    assert [a[3] for n, a in log if n.startswith('sbr_infonce') and n.endswith('_fwd')] == [1, 1]
    want = {'simgcl': [CLEAN] * 2 + [NOISY] * 4, 'xsimgcl': [NOISY] * 2}[kind]
    assert [n for n, _ in log if n.startswith('sbr_graph')] == want
    other = net.get_and_reset_other_loss()
    ref = R.model_torch(kind, g, uw, iw, u, i, labels, 2, torch.float64, seed=1, step=0, keep_layer=2)
    assert (ref['n_users'], ref['n_items']) == (n_u, n_i)
    for k in ('cl_u', 'cl_i', 'reg_loss'):
        assert abs(float(other[k]) - float(ref[k])) <= CL_RTOL * abs(float(ref[k])), k
    # the second forward is step 1: another noise
    net(torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV))
    again = net.get_and_reset_other_loss()
    assert net.step == 2 and float(again['cl_u']) != float(other['cl_u'])
    ref1 = R.model_torch(kind, g, uw, iw, u, i, labels, 2, torch.float64, seed=1, step=1, keep_layer=2)
    assert abs(float(again['cl_u']) - float(ref1['cl_u'])) <= CL_RTOL * abs(float(ref1['cl_u']))


# ---- 4. the Trainer, deterministic mode ----------------------------------------------------------------------------------------------------
def _train_5(kind, seed, noise_seed):
    Sm = S()
    Sm.reproducible(seed)
    ds = Sm.SyntheticDataset(300, 200, 5000, seed=1, n_negative_samples=3)
    net = Sm.ALGORITHMS[kind].build_from_conf({'embedding_dim': 24, 'n_layers': 2, 'seed': noise_seed}, ds)
    conf = {'learn': {'lr': 1e-2, 'wd': 1e-4, 'optimizer': 'adamw'}, 'run_settings': {'device': DEV}}
    tr = Sm.Trainer(net, None, None, _loss(200, 3), conf)
    assert tr.fused is None, 'the Trainer reaches autograd'
    net.train()
    it = iter(Sm.NegativeSamplingDataLoader(ds, batch_size=64, shuffle=True))
    before = Sm.ops.nondeterministic_launches()

    def steps():
        for _ in range(5):
            _, _, regs = tr.train_step(*next(it))
            assert set(regs) == {'reg_loss', 'cl_u', 'cl_i'} and float(regs['reg_loss']) > 0
        torch.cuda.synchronize()

    _, log = _logged(steps)
    names = [n for n, _ in log]
    # deterministic mode: the contrast (about 60 distinct rows of a batch of 64) takes InfoNCE's fixed-order entry, not the GEMM route
    assert names.count('sbr_infonce_fwd') == 10 and not any(n.startswith('sbr_infonce_gemm') for n in names)
    assert Sm.ops.nondeterministic_launches() == before and net.step == 5
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


@pytest.mark.parametrize('kind', ['simgcl', 'xsimgcl'])
def test_five_trainer_steps_twice_give_identical_tables(kind):
    Sm = S()
    prev = Sm.ops.is_deterministic()
    try:
        a, b, c = _train_5(kind, 3, 0), _train_5(kind, 3, 0), _train_5(kind, 3, 1)
    finally:
        Sm.ops.set_deterministic(prev)
    for k in a:
        _assert_bits(a[k], b[k], k)
    assert not torch.equal(a['user_embeddings.weight'], c['user_embeddings.weight']), 'another noise seed, other tables'


# ---- 5. evaluation ---------------------------------------------------------------------------------------------------------------------------
def test_the_evaluation_table_is_the_clean_mean_cached_and_rebuilt():
    g, uw, iw, u, i, labels = L.model_world(8)
    for kind in ('simgcl', 'xsimgcl'):
        net = _net(kind, g, uw, iw, 2, 1).eval()
        ud, items = torch.arange(40, device=DEV), torch.arange(30, device=DEV)

        def reps():
            def go():
                with torch.no_grad():
                    return net.get_user_representations(ud).clone(), net.get_item_representations(items).clone()
            out, log = _logged(go)
            names = [n for n, _ in log]
            assert NOISY not in names
            return out, names.count(CLEAN)

        def want():
            e0 = np.concatenate([net.user_embeddings.weight.detach().cpu().numpy(), net.item_embeddings.weight.detach().cpu().numpy()])
            e = R.mean32(g, e0, 2, 0.0, 0, 0, 0)[0]
            return t32(e[:40]), t32(e[40:])

        (a_u, a_i), n = reps()
        assert n == 2
        _assert_bits(a_u.cpu(), want()[0], 'first evaluation')
        _assert_bits(a_i.cpu(), want()[1], 'first evaluation')
        e0 = np.concatenate([uw, iw])
        with_layer_0 = L.mean64(g, e0, 2)
        assert float((a_u.cpu().double() - torch.from_numpy((3 * with_layer_0 - e0) / 2)[:40]).abs().max()) <= 1e-5, 'layers 1 .. L, not 0 .. L'
        assert float((a_u.cpu().double() - torch.from_numpy(with_layer_0)[:40]).abs().max()) > 1e-2, "not LightGCN's table"
        (_, _), n = reps()
        assert n == 0, 'a second evaluation propagates again'
        opt = torch.optim.SGD(net.parameters(), lr=0.5)
        logits = net(torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV))             # eval() mode: no noise, no contrast
        _loss(30, 4).compute_loss(logits, torch.from_numpy(labels).to(DEV)).backward()
        assert net.step == 0 and float(net.get_and_reset_other_loss()['reg_loss']) == 0
        opt.step()
        (b_u, b_i), n = reps()
        assert n == 2 and not torch.equal(b_u, a_u)
        _assert_bits(b_u.cpu(), want()[0], 'after the step')
        _assert_bits(b_i.cpu(), want()[1], 'after the step')
        net.train()
        net.eval()
        (c_u, _), n = reps()
        assert n == 2 and torch.equal(c_u, b_u), 'train() drops the table'
        with torch.no_grad():                                                               # training mode without a training forward: clean
            net.train()
            _assert_bits(net.get_user_representations(ud).cpu(), b_u.cpu(), 'training mode, outside forward')
        assert net.step == 0


class _EvalWorld:
    def __init__(self):
        Sm = S()
        self.ds = Sm.SyntheticDataset(600, 500, 12000, seed=4, n_negative_samples=3, holdout_per_user=1)
        self.g = L.Graph(self.ds.user_sampling_matrix_train)
        gen = torch.Generator().manual_seed(12)
        self.uw, self.iw = torch.randn(600, 64, generator=gen) * 0.5, torch.randn(500, 64, generator=gen) * 0.5
        self.net = _net('xsimgcl', self.g, self.uw.numpy(), self.iw.numpy(), 2, 1).eval()
        self.view = self.ds.eval_view()
        e0 = torch.cat([self.uw, self.iw]).numpy()
        e64 = torch.from_numpy(R.mean64(self.g, e0, 2, 0.0, 0, 0, 0)[0])
        bound = torch.from_numpy(R.clean_mean_bound(self.g, e0, 2))
        self.u64, self.i64, bu, bi = e64[:600], e64[600:], bound[:600], bound[600:]
        excluded = torch.from_numpy(self.view.exclude_data.toarray() != 0)
        self.masked = (self.u64 @ self.i64.t()).masked_fill(excluded, -float('inf')).to(DEV)
        # the scorer's tolerance on the representations it is given (scorer_truth_util), plus what the representations' own derived
        # error bound can move a score by
        self.tol = (T.C_TOL * 2.0 ** -24 * (self.u64.abs() @ self.i64.abs().t()) + bu @ self.i64.abs().t() + (self.u64.abs() + bu) @ bi.t()).to(DEV)

    def lists(self, scorer):
        Sm = S()
        ev = Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=(1, 10, 20)), dataset=self.view)
        got = []
        loader = type('L', (), {'dataset': self.view, 'batch_size': 256})()
        _, log = _logged(lambda: Sm.evaluation._score_split(self.net, loader, ev, DEV, scorer, 256, False, 32,
                                                            lambda s, u_, v, ix: got.append((v, ix))))
        return (torch.cat([g[0] for g in got]), torch.cat([g[1] for g in got])), [n for n, _ in log]


@pytest.fixture(scope='module')
def eval_world():
    return _EvalWorld()


@pytest.mark.parametrize('scorer', ['fp32', 'fp32_fused'])
def test_evaluation_lists_against_the_float64_ranking(eval_world, scorer):
    """600 users in chunks of 256, D = 64, as tests/test_hip_lightgcn.py: the top-20 lists of both routes against the float64 ranking of
    the clean layer-1..L table; the whole evaluation costs one propagation (L = 2 launches of the existing entry)"""
    w = eval_world
    w.net.train().eval()                                                                  # drops the cached table
    got, names = w.lists(scorer)
    assert names.count(CLEAN) == 2 and NOISY not in names, names.count(CLEAN)
    assert any(n.startswith('sbr_score_topk_f32s') for n in names) == (scorer == 'fp32_fused'), set(names)
    T.check_against_truth(got, torch.arange(600, device=DEV), w.masked, w.tol, 20, what=scorer)


# ---- 6. checkpoints, constructors, registry ----------------------------------------------------------------------------------------------------
def test_checkpoints_constructors_and_registry():
    Sm = S()
    g, uw, iw, u, i, labels = L.model_world(8)
    mf = Sm.SGDMatrixFactorization(40, 30, 8)
    lg = Sm.LightGCN(40, 30, g.m, embedding_dim=8, n_layers=2)
    for kind in ('simgcl', 'xsimgcl'):
        for src in (mf, lg):
            net = Sm.ALGORITHMS[kind](40, 30, g.m, embedding_dim=8)
            net.load_state_dict(src.state_dict())
            assert torch.equal(net.user_embeddings.weight, src.user_embeddings.weight)
            assert sorted(net.state_dict()) == sorted(src.state_dict())
        for kw in ({'eps': -0.1}, {'tau': 0.0}, {'cl_weight': -1.0}, {'n_layers': 0}):
            with pytest.raises(ValueError, match=next(iter(kw))):
                Sm.ALGORITHMS[kind](40, 30, g.m, **kw)
    for keep in (0, 3):
        with pytest.raises(ValueError, match='keep_layer'):
            Sm.XSimGCL(40, 30, g.m, n_layers=2, keep_layer=keep)
    assert Sm.ALGORITHMS['simgcl'] is Sm.SimGCL and Sm.ALGORITHMS['xsimgcl'] is Sm.XSimGCL
    ds = Sm.SyntheticDataset(30, 20, 200, seed=1, n_negative_samples=2)
    net = Sm.ALGORITHMS['xsimgcl'].build_from_conf({'embedding_dim': 8, 'n_layers': 3, 'keep_layer': 2}, ds).to(DEV).train()
    assert (net.n_layers, net.keep_layer, net.embedding_dim) == (3, 2, 8)
    uu, ii, _ = next(iter(Sm.NegativeSamplingDataLoader(ds, batch_size=16)))
    assert tuple(net(uu.to(DEV), ii.to(DEV)).shape) == tuple(ii.shape)
    with pytest.raises(RuntimeError, match='CUDA'):
        net(uu.to(DEV), ii)
    with pytest.raises(ValueError, match='training batch'):
        net(uu.to(DEV), ii.to(DEV)[:, 0])
