"""LightGCN on the GPU: the entry 'sbr_graph_propagate_f32' (csrc/graph_prop.hip) against its fp32 restatement bit for bit and against
float64 inside the derived bound (tests/lightgcn_ref.py), exact worlds, determinism over runs and row splits, refusals, and the model
(lightgcn.py) against float64 autograd, plain matrix factorisation, the Trainer and the evaluation routes.

Bit equality with the restatement is asked on EVERY input: lightgcn_ref.fma32 rounds the float64 sum to odd before the fp32 rounding, so
it has no double rounding and nothing falls back to the bound."""
from importlib import import_module

import numpy as np
import pytest
import torch

import lightgcn_ref as R
import scorer_truth_util as T
from hip_testutil import DEV, S, _Buf, _assert_bits, _assert_bound, call, stream

pytestmark = pytest.mark.gpu
ENTRY = 'sbr_graph_propagate_f32'


def _mod(name):
    return import_module(S().ops.__name__.rsplit('.', 1)[0] + '.' + name)


_CSR = {}


def dev_csr(g):
    if id(g) not in _CSR:
        _CSR[id(g)] = (g, _mod('features').DeviceCSR(g.m).to(DEV))
    return _CSR[id(g)][1]


_WORLDS = {}


def world(n_users, n_items):
    if (n_users, n_items) not in _WORLDS:
        _WORLDS[(n_users, n_items)] = R.world(n_users, n_items)
    return _WORLDS[(n_users, n_items)]


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def raw(g, x, y, s, scale, d, rows=None):
    """the entry itself on _Buf operands (any alignment)"""
    csr = dev_csr(g)
    ti, tx, _ = csr.transposed()
    r0, r1 = (0, g.n) if rows is None else rows
    call(ENTRY, csr.indptr.data_ptr(), csr.indices.data_ptr(), ti.data_ptr(), tx.data_ptr(), g.n_users, g.n_items, r0, r1, x.ptr, y.ptr,
         None if s is None else s.ptr, float(scale), d, stream())


# ---- 1. general worlds: the restatement bit for bit, float64 inside the bound -----------------------------------------------------------
@pytest.mark.parametrize('d', R.WIDTHS)
@pytest.mark.parametrize('n_items', R.ITEMS)
@pytest.mark.parametrize('n_users', R.USERS)
def test_propagate_against_restatement_and_float64(n_users, n_items, d):
    g = world(n_users, n_items)
    x, s0 = R.table(g.n, d, 1), R.table(g.n, d, 2)
    scale = 1.0 / 3
    y_ref, s_ref = R.propagate32(g, x, s0, scale)
    y64 = R.propagate64(g, x)
    s64 = (s0.astype(np.float64) + y64) * float(np.float32(scale))
    by, bs = R.propagate_bound(g, x, s0, scale)
    ops = S().ops
    xs, acc = t32(x).to(DEV), t32(s0).to(DEV)
    y = ops.graph_propagate(dev_csr(g), xs, sum=acc, sum_scale=scale)
    torch.cuda.synchronize()
    what = f'{n_users} x {n_items}, D = {d}'
    _assert_bits(y.cpu(), t32(y_ref), what + ': y against the restatement')
    _assert_bits(acc.cpu(), t32(s_ref), what + ': sum against the restatement')
    _assert_bound(y.cpu(), torch.from_numpy(y64), torch.from_numpy(by), what + ': y against float64')
    _assert_bound(acc.cpu(), torch.from_numpy(s64), torch.from_numpy(bs), what + ': sum against float64')
    assert torch.equal(xs.cpu(), t32(x))
    # without a sum; and the tables one float off the 16-byte boundary (the single-float kernels also where D % 4 == 0, with up to
    # eight chunks per lane at D = 512), inside NaN guards that must stay NaN
    y2 = ops.graph_propagate(dev_csr(g), xs)
    _assert_bits(y2.cpu(), t32(y_ref), what + ': y without a sum')
    bx, byy, bsum = _Buf(g.n, d, off=1, data=t32(x)), _Buf(g.n, d, off=1), _Buf(g.n, d, off=1, data=t32(s0))
    raw(g, bx, byy, bsum, scale, d)
    _assert_bits(byy.check_untouched(what=what + ': y off the boundary'), t32(y_ref), what + ': y off the boundary')
    _assert_bits(bsum.check_untouched(what=what + ': sum off the boundary'), t32(s_ref), what + ': sum off the boundary')


# ---- 2. exact worlds: float64 bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [1, 4, 5, 64, 260])
@pytest.mark.parametrize('with_empty', [False, True])
def test_exact_worlds_equal_float64(with_empty, d):
    g = R.exact_world(1, with_empty)
    e0 = R.int_table(g.n, d, 7)
    ops = S().ops
    x, acc = t32(e0).to(DEV), t32(e0).to(DEV)
    y = ops.graph_propagate(dev_csr(g), x, sum=acc, sum_scale=1.0)
    y64 = R.propagate64(g, e0)
    assert torch.equal(y.cpu().double(), torch.from_numpy(y64)), 'y'
    assert torch.equal(acc.cpu().double(), torch.from_numpy(e0 + y64)), 'sum'
    for n_layers in (1, 3):
        e = ops.LightGCNPropagateFn.apply(dev_csr(g), x, n_layers)
        assert torch.equal(e.cpu().double(), torch.from_numpy(R.mean64(g, e0, n_layers))), f'the scaled mean of {n_layers} layers'
    assert not bool(torch.signbit(y.cpu()[torch.from_numpy(g.deg == 0)]).any())


# ---- 3. determinism: runs, splits, rows outside the range -------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [3, 64, 65, 512])
def test_runs_and_row_splits_give_the_same_bits(d):
    g = world(257, 130)
    nu, n = g.n_users, g.n
    ops = S().ops
    x, s0 = t32(R.table(n, d, 1)).to(DEV), t32(R.table(n, d, 2)).to(DEV)
    acc = s0.clone()
    y = ops.graph_propagate(dev_csr(g), x, sum=acc, sum_scale=0.5)
    acc_b = s0.clone()
    _assert_bits(ops.graph_propagate(dev_csr(g), x, sum=acc_b, sum_scale=0.5).cpu(), y.cpu(), 'second run')
    _assert_bits(acc_b.cpu(), acc.cpu(), 'second run: sum')
    for cuts in ([0, nu, n], [0, 1, 100, nu - 3, nu + 7, n - 1, n], [0, 0, 63, 64, 65, n]):
        out, acc_c = torch.full((n, d), 7.25, device=DEV), s0.clone()
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            before_y, before_s = out.clone(), acc_c.clone()
            ops.graph_propagate(dev_csr(g), x, out=out, sum=acc_c, sum_scale=0.5, rows=(r0, r1))
            keep = torch.ones(n, dtype=torch.bool, device=DEV)
            keep[r0:r1] = False
            assert torch.equal(out[keep], before_y[keep]) and torch.equal(acc_c[keep], before_s[keep]), f'rows outside [{r0}, {r1}) were written'
        _assert_bits(out.cpu(), y.cpu(), f'split {cuts}')
        _assert_bits(acc_c.cpu(), acc.cpu(), f'split {cuts}: sum')
    part = ops.graph_propagate(dev_csr(g), x, rows=(nu - 2, nu + 2))                     # a new result: zeros outside the range
    assert torch.equal(part[nu - 2:nu + 2], y[nu - 2:nu + 2]) and not bool(part[:nu - 2].any()) and not bool(part[nu + 2:].any())


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    Sm = S()
    g = world(5, 64)
    n, d = g.n, 8
    x, y, s = _Buf(n, d, data=t32(R.table(n, d, 1))), _Buf(n, d, fill=7.25), _Buf(n, d, fill=-3.5)
    wide = _Buf(n, 513, fill=1.0)

    def untouched():
        assert bool((y.check_untouched() == 7.25).all()) and bool((s.check_untouched() == -3.5).all())
        assert torch.equal(x.check_untouched(), t32(R.table(n, d, 1)))

    for args, text in (((g, x, x, s, 1.0, d), 'x aliases y'), ((g, x, y, x, 1.0, d), 'x aliases sum'), ((g, x, y, y, 1.0, d), 'y aliases sum'),
                       ((g, x, y, s, 1.0, 0), r'D=0 outside \[1, 512\]'), ((g, wide, wide, None, 1.0, 513), r'D=513 outside \[1, 512\]'),
                       ((g, x, y, s, 1.0, d, (0, n + 1)), r'row range \[0, 70\) outside \[0, 69\]'),
                       ((g, x, y, s, 1.0, d, (3, 2)), 'row range'), ((g, x, y, s, 1.0, d, (-1, 2)), 'row range')):
        with pytest.raises(Sm.SibrarHipError, match=text):
            raw(*args)
        untouched()
    # overlapping, not identical: x shifted by one row into y's storage
    both = torch.zeros((n + 1) * d, device=DEV)
    csr = dev_csr(g)
    ti, tx, _ = csr.transposed()
    with pytest.raises(Sm.SibrarHipError, match='x aliases y'):
        call(ENTRY, csr.indptr.data_ptr(), csr.indices.data_ptr(), ti.data_ptr(), tx.data_ptr(), 5, 64, 0, n, both.data_ptr(),
             both.data_ptr() + 4 * d, None, 1.0, d, stream())
    assert not bool(both.any())
    for k in (0, 2, 8, 9):
        ptrs = [csr.indptr.data_ptr(), csr.indices.data_ptr(), ti.data_ptr(), tx.data_ptr(), 5, 64, 0, n, x.ptr, y.ptr, s.ptr, 1.0, d, stream()]
        ptrs[k] = None
        with pytest.raises(Sm.SibrarHipError, match='null operand'):
            call(ENTRY, *ptrs)
    raw(g, x, y, s, 1.0, d, (4, 4))                                                       # an empty range is a no-op
    untouched()
    # ops: a matrix with values, wrong tables
    weighted = g.m.copy()
    weighted.data[:] = 0.5
    xs = x.t.contiguous()
    with pytest.raises(ValueError, match='0/1'):
        Sm.ops.graph_propagate(_mod('features').DeviceCSR(weighted).to(DEV), xs)
    with pytest.raises(ValueError, match='contiguous float32'):
        Sm.ops.graph_propagate(csr, xs[:-1])
    with pytest.raises(ValueError, match='contiguous float32'):
        Sm.ops.graph_propagate(csr, xs.double())
    with pytest.raises(ValueError, match='contiguous float32'):
        Sm.ops.graph_propagate(csr, xs, out=torch.empty(n, d + 1, device=DEV)[:, :d])
    with pytest.raises(Sm.SibrarHipError, match='x aliases y'):
        Sm.ops.graph_propagate(csr, xs, out=xs)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Sm.ops.graph_propagate(csr, xs.cpu())


# ---- 5. the model against float64 -------------------------------------------------------------------------------------------------------------
def _loss(n_items, neg):
    return S().RecBayesianPersonalizedRankingLoss(n_items=n_items, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=neg)


def _net(g, uw, iw, n_layers):
    net = S().LightGCN(g.n_users, g.n_items, g.m, embedding_dim=uw.shape[1], n_layers=n_layers)
    net.load_state_dict({'user_embeddings.weight': t32(uw), 'item_embeddings.weight': t32(iw)})
    return net.to(DEV)


@pytest.mark.parametrize('d', [8, 64])
@pytest.mark.parametrize('n_layers', [0, 1, 3])
def test_model_logits_loss_and_gradients_against_float64(n_layers, d):
    """Tolerance: 8 x the error of the same formula in torch float32 on the CPU against float64 on these inputs (lightgcn_ref.yardstick:
    the maximum absolute error of the quantity as measured, no floor), for the logits, the loss and both table gradients alike. Both
    figures of every quantity, measured on an MI355X, are recorded in DESIGN.md 4.29."""
    g, uw, iw, u, i, labels = R.model_world(d)
    ref = R.model_torch(g, uw, iw, u, i, labels, n_layers, torch.float64)
    cpu = R.model_torch(g, uw, iw, u, i, labels, n_layers, torch.float32)
    net = _net(g, uw, iw, n_layers).train()
    logits = net(torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV))
    loss = _loss(30, 4).compute_loss(logits, torch.from_numpy(labels).to(DEV))
    loss.backward()
    got = {'logits': logits.detach(), 'loss': loss.detach().reshape(()), **{k: p.grad for k, p in net.named_parameters()}}
    worst = []
    for k in ('logits', 'loss', 'user_embeddings.weight', 'item_embeddings.weight'):
        e_cpu = R.yardstick(ref[k], cpu[k])
        err = float((got[k].cpu().double().reshape(ref[k].shape) - ref[k]).abs().max())
        print(f'L={n_layers} D={d} {k}: error {err:.3e}, float32 on the CPU {e_cpu:.3e}, allowed {R.FACTOR * e_cpu:.3e}')
        worst.append((k, err, R.FACTOR * e_cpu))
    for k, err, tol in worst:
        assert err <= tol, f'{k}: error {err:.3e} over 8 x the float32 CPU error = {tol:.3e}'


def test_zero_layers_equals_matrix_factorisation_bit_for_bit():
    g, uw, iw, u, i, labels = R.model_world(64)
    net = _net(g, uw, iw, 0).train()
    mf = S().SGDMatrixFactorization(40, 30, 64)
    mf.load_state_dict(net.state_dict())
    mf = mf.to(DEV).train()
    ud, idd = torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV)
    L = _mod('_lib')
    L.CALL_LOG = []
    try:
        a = net(ud, idd)
        names = [n for n, _ in L.CALL_LOG]
    finally:
        L.CALL_LOG = None
    assert ENTRY not in names, 'L = 0 launches no propagation'
    _assert_bits(a.detach().cpu(), mf(ud, idd).detach().cpu(), 'training logits')
    net.eval(), mf.eval()
    with torch.no_grad():
        items = torch.arange(30, device=DEV)
        a = net.combine_user_item_representations(net.get_user_representations(ud), net.get_item_representations(items))
        b = mf.combine_user_item_representations(mf.get_user_representations(ud), mf.get_item_representations(items))
    _assert_bits(a.cpu(), b.cpu(), 'all-pairs scores')
    e0 = torch.randn(70, 8, device=DEV, requires_grad=True)
    out = S().ops.LightGCNPropagateFn.apply(dev_csr(g), e0, 0)
    assert torch.equal(out, e0)
    out.sum().backward()
    assert torch.equal(e0.grad, torch.ones_like(e0))


def test_backward_is_the_same_operator_on_the_gradient():
    g = world(257, 64)
    ops = S().ops
    e0 = t32(R.table(g.n, 12, 5)).to(DEV).requires_grad_()
    w = t32(R.table(g.n, 12, 6)).to(DEV)
    before = ops.nondeterministic_launches()
    (ops.LightGCNPropagateFn.apply(dev_csr(g), e0, 3) * w).sum().backward()
    _assert_bits(e0.grad.cpu(), t32(R.mean32(g, w.cpu().numpy(), 3)), 'gradient against the restatement applied to the incoming gradient')
    assert ops.nondeterministic_launches() == before


# ---- 6. the Trainer, deterministic mode, evaluation ---------------------------------------------------------------------------------------------
def _train_5(seed):
    Sm = S()
    Sm.reproducible(seed)
    ds = Sm.SyntheticDataset(300, 200, 5000, seed=1, n_negative_samples=3)
    net = Sm.ALGORITHMS['lightgcn'].build_from_conf({'embedding_dim': 24, 'n_layers': 2}, ds)
    conf = {'learn': {'lr': 1e-2, 'wd': 1e-4, 'optimizer': 'adamw'}, 'run_settings': {'device': DEV}}
    tr = Sm.Trainer(net, None, None, _loss(200, 3), conf)
    net.train()
    it = iter(Sm.NegativeSamplingDataLoader(ds, batch_size=64, shuffle=True))
    before = Sm.ops.nondeterministic_launches()
    for _ in range(5):
        tr.train_step(*next(it))
    torch.cuda.synchronize()
    assert Sm.ops.nondeterministic_launches() == before
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def test_five_trainer_steps_twice_give_identical_tables():
    Sm = S()
    prev = Sm.ops.is_deterministic()
    try:
        a, b, c = _train_5(3), _train_5(3), _train_5(4)
    finally:
        Sm.ops.set_deterministic(prev)
    for k in a:
        _assert_bits(a[k], b[k], k)
    assert not torch.equal(a['user_embeddings.weight'], c['user_embeddings.weight'])
    torch.manual_seed(3)
    init = Sm.LightGCN(300, 200, Sm.SyntheticDataset(300, 200, 5000, seed=1, n_negative_samples=3).user_sampling_matrix_train, 24, 2)
    assert float((a['item_embeddings.weight'] - init.item_embeddings.weight.detach()).abs().max()) > 1e-3, 'the steps moved the tables'


class _EvalWorld:
    def __init__(self):
        Sm = S()
        self.ds = Sm.SyntheticDataset(600, 500, 12000, seed=4, n_negative_samples=3, holdout_per_user=1)
        self.g = R.Graph(self.ds.user_sampling_matrix_train)
        gen = torch.Generator().manual_seed(12)
        self.uw, self.iw = torch.randn(600, 64, generator=gen) * 0.5, torch.randn(500, 64, generator=gen) * 0.5
        self.net = _net(self.g, self.uw.numpy(), self.iw.numpy(), 2).eval()
        self.view = self.ds.eval_view()
        e0 = torch.cat([self.uw, self.iw]).numpy()
        e64, bound = torch.from_numpy(R.mean64(self.g, e0, 2)), torch.from_numpy(R.mean_bound(self.g, e0, 2))
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


@pytest.mark.parametrize('scorer', ['fp32', 'fp32_fused'])
def test_evaluation_lists_against_the_float64_ranking(eval_world, scorer):
    """600 users in chunks of 256 (three chunks), D = 64: the top-20 lists of both routes against the float64 ranking with the near-tie
    acceptance of tests/scorer_truth_util.py; the whole evaluation costs one propagation (L = 2 launches), not one per chunk"""
    w = eval_world
    w.net.train().eval()                                                                  # drops the cached table
    got, names = w.lists(scorer)
    assert names.count(ENTRY) == 2, names.count(ENTRY)
    assert any(n.startswith('sbr_score_topk_f32s') for n in names) == (scorer == 'fp32_fused'), set(names)
    T.check_against_truth(got, torch.arange(600, device=DEV), w.masked, w.tol, 20, what=scorer)
    res = S().evaluate_recommender_algorithm(w.net, type('L', (), {'dataset': w.view, 'batch_size': 256})(),
                                             S().FullEvaluator(config=S().evaluation._Cfg(top_k=(10,)), dataset=w.view), DEV, scorer=scorer)
    assert 0.0 <= res['ndcg@10'] <= 1.0


def test_the_evaluation_cache_is_rebuilt_when_the_tables_change():
    Sm = S()
    g, uw, iw, u, i, labels = R.model_world(8)
    net = _net(g, uw, iw, 2).eval()
    ud = torch.arange(40, device=DEV)
    L = _mod('_lib')

    def reps():
        L.CALL_LOG = []
        try:
            with torch.no_grad():
                out = net.get_user_representations(ud).clone(), net.get_item_representations(torch.arange(30, device=DEV)).clone()
            return out, [n for n, _ in L.CALL_LOG].count(ENTRY)
        finally:
            L.CALL_LOG = None

    def want():
        e = R.mean32(g, np.concatenate([net.user_embeddings.weight.detach().cpu().numpy(), net.item_embeddings.weight.detach().cpu().numpy()]), 2)
        return t32(e[:40]), t32(e[40:])

    (a_u, a_i), n = reps()
    assert n == 2
    _assert_bits(a_u.cpu(), want()[0], 'first evaluation')
    _assert_bits(a_i.cpu(), want()[1], 'first evaluation')
    (_, _), n = reps()
    assert n == 0, 'a second evaluation propagates again'
    # an optimizer step in eval() mode (torch's: it bumps the tables' version counters)
    opt = torch.optim.SGD(net.parameters(), lr=0.5)
    _loss(30, 4).compute_loss(net(torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV)), torch.from_numpy(labels).to(DEV)).backward()
    opt.step()
    (b_u, b_i), n = reps()
    assert n == 2 and not torch.equal(b_u, a_u)
    _assert_bits(b_u.cpu(), want()[0], 'after the step')
    _assert_bits(b_i.cpu(), want()[1], 'after the step')
    # the engine's optimizer writes through raw pointers, which no version counter sees: it drops the table itself on every step.
    # Stepped by hand, the model in eval() mode throughout, no train() in between
    fused = Sm.FusedOptimizer(net, 'adam', 1e-1, 0.)
    (r_u, _), n = reps()
    assert n == 2 and torch.equal(r_u, b_u), 'moving the tables into the flat buffer changes their storage, not their values'
    (_, _), n = reps()
    assert n == 0
    fused.zero_grad()
    _loss(30, 4).compute_loss(net(torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV)), torch.from_numpy(labels).to(DEV)).backward()
    versions = net._cache_key()
    fused.step()
    assert net._cache_key() == versions and not net.training, 'the step is invisible to the version counters: the optimizer has to say'
    (c_u, c_i), n = reps()
    assert n == 2 and not torch.equal(c_u, b_u)
    _assert_bits(c_u.cpu(), want()[0], 'after the fused optimizer step')
    _assert_bits(c_i.cpu(), want()[1], 'after the fused optimizer step')
    # and through the Trainer
    conf = {'learn': {'lr': 1e-1, 'wd': 0., 'optimizer': 'adam'}, 'run_settings': {'device': DEV}}
    tr = Sm.Trainer(net, None, None, _loss(30, 4), conf)
    net.train()
    tr.train_step(torch.from_numpy(u), torch.from_numpy(i), torch.from_numpy(labels))
    net.eval()
    (t_u, t_i), n = reps()
    assert n == 2 and not torch.equal(t_u, c_u)
    _assert_bits(t_u.cpu(), want()[0], 'after the Trainer step')
    _assert_bits(t_i.cpu(), want()[1], 'after the Trainer step')
    # load_state_dict
    net.load_state_dict({'user_embeddings.weight': t32(uw), 'item_embeddings.weight': t32(iw)})
    (d_u, d_i), n = reps()
    assert n == 2
    _assert_bits(d_u.cpu(), a_u.cpu(), 'after load_state_dict')
    _assert_bits(d_i.cpu(), a_i.cpu(), 'after load_state_dict')
    # with gradients enabled the table is computed afresh and stays on the tape
    assert net.get_user_representations(ud).requires_grad
