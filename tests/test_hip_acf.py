"""ACF (acf) on the GPU: the product class against the G19 fixture of the real reference, the fused anchor-mixing kernels against float64
under the three-way criterion of tests/test_hip_c1.py and tests/test_hip_protomf.py

    err(GPU, truth) <= KAPPA * max(err(torch-CPU fp32, 16 threads), err(torch-CPU fp32, 1 thread)) + REL_FLOOR * ||truth||

(err = 2-norm of the difference per tensor; KAPPA and REL_FLOOR are those files' values; the measured ratios are printed), duplicate rows,
the reference's NaN at an empty anchor, the range errors, the deterministic mode, full-catalogue evaluation on all three scorer routes and
one end-to-end fit."""
import json
import os
from importlib import import_module

import numpy as np
import pytest
import torch

import acf_ref
from golden_util import GOLDEN, I, close, host_dataset, load, state_dict, world
import scorer_truth_util as T

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = dict(rtol=1e-4, atol=1e-5)                                 # tests/test_hip_protomf.py
CASES = json.load(open(os.path.join(GOLDEN, 'g19_acf.json')))['cases']
KAPPA = 3.0                                                      # tests/test_hip_c1.py, tests/test_hip_protomf.py
REL_FLOOR = 1e-7
THREADS = torch.get_num_threads()
W_EXC, W_INC = 0.7, 1.3                                          # regulariser weights of the kernel tests (unequal, both of order 1)


def S():
    import sibrar_amd
    return sibrar_amd


def _lib():
    return import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')


def _loss(kind, n_items=I, neg=3):
    cls = {'bce': S().RecBinaryCrossEntropy, 'bpr': S().RecBayesianPersonalizedRankingLoss}[kind]
    return cls(n_items=n_items, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=neg)


def _err(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm())


class Report:
    def __init__(self, title):
        self.title, self.lines, self.bad, self.worst = title, [], [], {}

    def kappa(self, what, gpu, cpu16, cpu1, truth, group=None):
        assert bool(torch.isfinite(gpu).all()), f'{what}: not finite'
        e_gpu, e16, e1 = _err(gpu, truth), _err(cpu16, truth), _err(cpu1, truth)
        floor = REL_FLOOR * float(truth.double().norm())
        cpu = max(e16, e1)
        ok = e_gpu <= KAPPA * cpu + floor
        ratio = e_gpu / cpu if cpu > 0 else (0.0 if e_gpu == 0 else float('inf'))
        line = f'{what:<60} gpu {e_gpu:.3e}  cpu16 {e16:.3e}  cpu1 {e1:.3e}  ratio {ratio:6.2f}  floor {floor:.2e}{"" if ok else "  FAIL"}'
        self.lines.append(line)
        self.worst[group or what] = max(self.worst.get(group or what, 0.0), ratio)
        if not ok:
            self.bad.append(line)

    def finish(self):
        print(f'\n== {self.title}')
        print('\n'.join(self.lines))
        print('largest ratio per tensor:', {k: round(v, 2) for k, v in self.worst.items()})
        assert not self.bad, f'{self.title}: {len(self.bad)} comparison(s) fail:\n' + '\n'.join(self.bad)


def _with_threads(n, fn):
    torch.set_num_threads(n)
    try:
        return fn()
    finally:
        torch.set_num_threads(THREADS)


# ---- 1. golden parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_g19_acf_on_hip_kernels(case):
    """The product class == the real reference on every G19 case: train-mode logits, every loss-dictionary entry, BCE and BPR loss,
    every gradient of rec_loss + reg_loss under each loss, evaluation scores through get_*_representations + combine, the pre_tune /
    post_tune outputs of both sides, post_val."""
    z = load('g19_acf')
    name = case['name']
    m = S().ALGORITHMS['acf'].build_from_conf(case['conf'], host_dataset(world(z)))
    sd = state_dict(z, f'{name}/sd/')
    assert list(m.state_dict().keys()) == list(sd.keys()) == case['keys']
    m.load_state_dict(sd)
    m.to(DEV).train()
    u, i, labels = (torch.from_numpy(z[k]).to(DEV) for k in ('u', 'i', 'labels'))
    for kind in ('bce', 'bpr'):
        m.zero_grad()
        logits = m(u, i)
        close(logits.detach().cpu(), z[f'{name}/logits'], what='logits', **TOL)
        loss = _loss(kind).compute_loss(logits, labels)
        close(loss.detach().cpu(), z[f'{name}/loss_{kind}'], what=f'{kind} loss', **TOL)
        other = m.get_and_reset_other_loss()
        assert list(other) == case['other_keys'] == ['reg_loss', 'exc_loss', 'inc_loss']
        for k, v in other.items():
            assert v.is_cuda, f'{k} left the device'
            close(v.detach().cpu(), z[f'{name}/other_{kind}/{k}'], what=f'{kind} {k}', **TOL)
        (loss + other['reg_loss']).backward()
        for k, p in m.named_parameters():
            close(p.grad.cpu(), z[f'{name}/grad_{kind}/{k}'], what=f'{kind} grad {k}', rtol=1e-4, atol=1e-6, norm_rtol=1e-4)
    m.eval()
    with torch.no_grad():
        ir = m.get_item_representations(torch.arange(I, device=DEV))
        assert len(ir) == 3 and ir[2] is None
        scores = m.combine_user_item_representations(m.get_user_representations(u), ir)
        close(scores.cpu(), z[f'{name}/scores_all'], what='all-pairs scores', **TOL)
        c_u, c_i = m.get_user_representations_pre_tune(u), m.get_item_representations_pre_tune(i)
        close(c_u.cpu(), z[f'{name}/user_pre_tune'], what='user pre_tune', **TOL)
        close(c_i.cpu(), z[f'{name}/item_pre_tune'], what='item pre_tune', **TOL)
        close(m.get_user_representations_post_tune(c_u).cpu(), z[f'{name}/user_post_tune'], what='user post_tune', **TOL)
        i_post = m.get_item_representations_post_tune(c_i)
        assert len(i_post) == 3 and i_post[1] is c_i and i_post[2] is None
        close(i_post[0].cpu(), z[f'{name}/item_post_tune'], what='item post_tune', **TOL)
    pv = m.post_val(0)
    assert list(pv) == list(case['post_val']) and all(isinstance(v, float) for v in pv.values())
    for k, v in pv.items():
        close(torch.tensor(v), torch.tensor(case['post_val'][k]), what=f'post_val {k}', **TOL)


# ---- 2. the kernels against float64 -------------------------------------------------------------------------------------------------
def _inputs(R, D, K, seed, n_table=None):
    gen = torch.Generator().manual_seed(seed)
    n_table = n_table or R
    table, anchors = torch.randn(n_table, D, generator=gen), torch.randn(K, D, generator=gen)
    if n_table == R:
        rows = torch.randperm(R, generator=gen).to(torch.int32)
    else:
        rows = torch.randint(0, n_table, (R,), generator=gen).to(torch.int32)
    G = torch.randn(R, D, generator=gen) / R
    return table, rows, anchors, G


def _mix_cpu(table, rows, anchors, G, dtype, with_losses=True):
    """(r, c, exc, inc, d table, dA) of sum(r * G) + W_EXC exc + W_INC inc by torch autograd"""
    t, a = table.to(dtype).clone().requires_grad_(True), anchors.to(dtype).clone().requires_grad_(True)
    r, c, s = acf_ref.mix(t[rows.long()], a)
    exc, inc = acf_ref.losses(c, s)
    obj = (r * G.to(dtype)).sum()
    if with_losses:
        obj = obj + W_EXC * exc + W_INC * inc
    obj.backward()
    return r.detach(), c.detach(), exc.detach().reshape(1), inc.detach().reshape(1), t.grad, a.grad


def _mix_gpu(table, rows, anchors, G, with_losses=True):
    t, a = table.to(DEV).requires_grad_(True), anchors.to(DEV).requires_grad_(True)
    r, c, exc, inc = S().ops.AnchorMixFn.apply(t, rows.to(DEV), a, with_losses)
    assert not c.requires_grad
    obj = (r * G.to(DEV)).sum()
    if with_losses:
        obj = obj + W_EXC * exc + W_INC * inc
    obj.backward()
    torch.cuda.synchronize()
    return r.detach().cpu(), c.detach().cpu(), exc.detach().cpu().reshape(1), inc.detach().cpu().reshape(1), t.grad.cpu(), a.grad.cpu()


NAMES = ('r', 'c', 'exc', 'inc', 'dE', 'dA')


def _row_cap_rows():
    """the smallest row count at which a workgroup of the kernels walks two row tiles (the grid cap times the tile height, plus one
    row), plus 5"""
    ops = S().ops
    return ops.ANCHOR_MAX_WG * ops.ANCHOR_TILE + 1 + 5


@pytest.mark.parametrize('R,D,K', [(37, 100, 20), (130, 33, 70), (2048, 64, 130), (512, 512, 256), (3, 1, 2), ('row_cap', 5, 3)])
def test_anchor_mix_kernels_against_float64(R, D, K):
    """r, c, both losses, dE and dA of ops.AnchorMixFn against torch autograd in float64. The rows are a permutation of the table, so the
    table gradient is dE read back through the lookup. (512, 512, 256): c has exact zeros in fp32 (asserted): a backward pass that took
    log c would be NaN there. The row-cap shape runs the grid-stride loop with the largest number of cross-workgroup partials."""
    if R == 'row_cap':
        R = _row_cap_rows()
        assert S().lib().sbr_anchor_mix_workspace(R, D, K, 0) == S().lib().sbr_anchor_mix_workspace(R - 6, D, K, 0) > 0
    table, rows, anchors, G = _inputs(R, D, K, seed=R + D + K)
    truth = _mix_cpu(table, rows, anchors, G, torch.float64)
    q = acf_ref.q_of(truth[1])
    assert float(q.min()) > 0, 'precondition: every anchor takes some mass in float64'
    cpu16 = _with_threads(16, lambda: _mix_cpu(table, rows, anchors, G, torch.float32))
    cpu1 = _with_threads(1, lambda: _mix_cpu(table, rows, anchors, G, torch.float32))
    if (R, D, K) == (512, 512, 256):
        assert bool((cpu1[1] == 0).any()), 'precondition: c has exact zeros in fp32'
    gpu = _mix_gpu(table, rows, anchors, G)
    rep = Report(f'anchor_mix R={R} D={D} K={K} (q min {float(q.min()):.2e})')
    for n, what in enumerate(NAMES):
        rep.kappa(what, gpu[n], cpu16[n], cpu1[n], truth[n])
    rep.finish()


def test_anchor_mix_user_side_form_against_float64():
    """no losses, g_exc = g_inc = None: r, c, dE and dA of sum(r * G) alone; the loss outputs are zeros"""
    R, D, K = 37, 100, 20
    table, rows, anchors, G = _inputs(R, D, K, seed=5)
    truth = _mix_cpu(table, rows, anchors, G, torch.float64, False)
    cpu16 = _with_threads(16, lambda: _mix_cpu(table, rows, anchors, G, torch.float32, False))
    cpu1 = _with_threads(1, lambda: _mix_cpu(table, rows, anchors, G, torch.float32, False))
    gpu = _mix_gpu(table, rows, anchors, G, False)
    assert float(gpu[2]) == 0. and float(gpu[3]) == 0.
    rep = Report('anchor_mix user side')
    for n in (0, 1, 4, 5):
        rep.kappa(NAMES[n], gpu[n], cpu16[n], cpu1[n], truth[n])
    rep.finish()
    ops = S().ops
    t, a, idx = table.to(DEV), anchors.to(DEV), rows.to(DEV)
    assert torch.equal(ops.anchor_mix(t, idx, a).cpu(), gpu[0]) and torch.equal(ops.anchor_mix(t, idx, a, want='c').cpu(), gpu[1])
    assert torch.equal(ops.anchor_mix(t, None, a)[idx.long()].cpu(), gpu[0])


@pytest.mark.parametrize('deterministic', [False, True], ids=['default', 'deterministic'])
def test_anchor_mix_duplicate_rows_at_the_table_gradient(deterministic):
    """300 rows drawn from a 40-row table: the scattered TABLE gradient against float64, in both modes"""
    ops = S().ops
    table, rows, anchors, G = _inputs(300, 24, 6, seed=77, n_table=40)
    truth = _mix_cpu(table, rows, anchors, G, torch.float64)
    assert float(acf_ref.q_of(truth[1]).min()) > 0
    cpu16 = _with_threads(16, lambda: _mix_cpu(table, rows, anchors, G, torch.float32))
    cpu1 = _with_threads(1, lambda: _mix_cpu(table, rows, anchors, G, torch.float32))
    prev = ops.set_deterministic(deterministic)
    try:
        ops.nondeterministic_launches(reset=True)
        gpu = _mix_gpu(table, rows, anchors, G)
        if deterministic:
            assert ops.nondeterministic_launches() == 0
    finally:
        ops.set_deterministic(prev)
    rep = Report(f'anchor_mix with duplicate rows (deterministic = {deterministic})')
    for n, what in enumerate(('r', 'c', 'exc', 'inc', 'd table', 'dA')):
        rep.kappa(what, gpu[n], cpu16[n], cpu1[n], truth[n])
    rep.finish()


# ---- 4. the NaN contract ----------------------------------------------------------------------------------------------------------------
def test_an_empty_anchor_gives_nan_inc_and_nothing_else():
    """logits (200, 0) in every row: c = [1, 0], q = [1, 0], inc = NaN as in the reference (0 log 0); r, c and exc are finite and equal
    the restatement. An arithmetic result, not a fault."""
    table, anchors = acf_ref.nan_case(torch.float32)
    r_ref, c_ref, s_ref = acf_ref.mix(table, anchors)
    exc_ref, inc_ref = acf_ref.losses(c_ref, s_ref)
    assert bool(torch.isnan(inc_ref))
    r, c, exc, inc = S().ops.AnchorMixFn.apply(table.to(DEV), torch.arange(4, device=DEV), anchors.to(DEV), True)
    assert bool(torch.isnan(inc))
    assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(c).all()) and bool(torch.isfinite(exc))
    assert torch.equal(c.cpu(), c_ref) and torch.equal(r.cpu(), r_ref) and float(exc) == float(exc_ref) == 0.


# ---- 5. range errors, R = 0 ---------------------------------------------------------------------------------------------------------------
def test_anchor_mix_shapes_outside_the_range_raise_and_no_rows_is_legal():
    ops = S().ops
    for D, K in ((513, 20), (100, 1), (100, 257)):
        with pytest.raises(ValueError, match='n_anchors'):
            ops.anchor_mix(torch.zeros(3, D, device=DEV), None, torch.zeros(K, D, device=DEV))
    L = _lib()
    x = torch.zeros(4, 8, device=DEV)
    with pytest.raises(S().SibrarHipError, match='n_anchors'):         # the entry points themselves refuse through sbr_last_error
        L.call('sbr_anchor_mix_fwd', x.data_ptr(), 8, None, 4, 8, x.data_ptr(), 1, x.data_ptr(), None, None, None, None, None, None, None,
               0, L.stream())
    with pytest.raises(S().SibrarHipError, match='n_anchors'):
        L.call('sbr_anchor_mix_bwd', x.data_ptr(), None, None, x.data_ptr(), 8, None, 4, 8, x.data_ptr(), 257, x.data_ptr(), None, None,
               x.data_ptr(), None, None, 0, L.stream())
    none = torch.zeros(0, dtype=torch.long, device=DEV)
    assert tuple(ops.anchor_mix(x, none, x).shape) == (0, 8) and tuple(ops.anchor_mix(x, none, x, want='c').shape) == (0, 4)
    t, a = torch.randn(5, 8, device=DEV, requires_grad=True), torch.randn(4, 8, device=DEV, requires_grad=True)
    L.CALL_LOG = []
    try:
        r, c, exc, inc = ops.AnchorMixFn.apply(t, none.reshape(0, 3), a, True)
        assert tuple(r.shape) == (0, 3, 8) and tuple(c.shape) == (0, 3, 4) and float(exc) == 0. and float(inc) == 0.
        (r.sum() + exc + inc).backward()
        names = [n for n, _ in L.CALL_LOG]
    finally:
        L.CALL_LOG = None
    assert 'sbr_anchor_mix_fwd' not in names
    assert tuple(t.grad.shape) == (5, 8) and tuple(a.grad.shape) == (4, 8) and not bool(t.grad.any()) and not bool(a.grad.any())


# ---- 6. deterministic mode ----------------------------------------------------------------------------------------------------------------
def _train_20(seed):
    Sm = S()
    Sm.reproducible(seed)
    ds = Sm.SyntheticDataset(2000, 3000, 60000, seed=1, n_negative_samples=3)
    net = Sm.ACF(2000, 3000, 64, 20)
    conf = {'learn': {'lr': 1e-3, 'wd': 1e-4, 'optimizer': 'adamw'}, 'run_settings': {'device': DEV}}
    tr = Sm.Trainer(net, None, None, _loss('bpr', 3000), conf)
    net.train()
    it = iter(Sm.NegativeSamplingDataLoader(ds, batch_size=256, shuffle=True))
    for _ in range(20):
        tr.train_step(*next(it))
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def test_acf_deterministic_training_is_bit_identical():
    ops = S().ops
    prev = ops.is_deterministic()
    try:
        ops.nondeterministic_launches(reset=True)
        a = _train_20(123)
        b = _train_20(123)
        assert ops.nondeterministic_launches() == 0
        assert ops.is_deterministic()
        init = S().ACF(2000, 3000, 64, 20).state_dict()
        for k in a:
            assert torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)), k
            assert bool(torch.isfinite(a[k]).all()) and tuple(a[k].shape) == tuple(init[k].shape)
    finally:
        ops.set_deterministic(prev)


# ---- 7. evaluation ----------------------------------------------------------------------------------------------------------------------
ROUTE_C = {'fp32': 72.0, 'fp32_fused': 72.0, 'fp16_fused': 2.0 ** 14 + 72.0}      # tests/test_hip_protomf.py


class _EvalWorld:
    def __init__(self, embedding_dim):
        Sm = S()
        self.ds = Sm.SyntheticDataset(2000, 3000, 60000, seed=4, n_negative_samples=3, holdout_per_user=1)
        torch.manual_seed(11)
        self.net = Sm.ACF(2000, 3000, embedding_dim, 20)
        gen = torch.Generator().manual_seed(12)
        self.net.load_state_dict({k: torch.randn(v.shape, generator=gen) * 0.5 for k, v in self.net.state_dict().items()})
        self.net.to(DEV).eval()
        self.view = self.ds.eval_view()
        sd = {k: v.detach().cpu().double() for k, v in self.net.state_dict().items()}
        with torch.no_grad():
            self.u64 = acf_ref.side(sd, 'user', torch.arange(2000))[0]
            self.i64 = acf_ref.side(sd, 'item', torch.arange(3000))[0]
            self.scores = acf_ref.combine(self.u64, self.i64).to(DEV)
        self.excluded = torch.from_numpy(self.view.exclude_data.toarray() != 0).to(DEV)
        self.masked = self.scores.masked_fill(self.excluded, -float('inf'))

    def lists(self, scorer, top_k=(1, 10, 20)):
        Sm = S()
        ev = Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=top_k), dataset=self.view)
        got = []
        loader = type('L', (), {'dataset': self.view, 'batch_size': 512})()
        L = _lib()
        L.CALL_LOG = []
        try:
            Sm.evaluation._score_split(self.net, loader, ev, DEV, scorer, None, False, 32, lambda s, u_, v, ix: got.append((v, ix)))
            names = {n for n, _ in L.CALL_LOG}
        finally:
            L.CALL_LOG = None
        return (torch.cat([g[0] for g in got]), torch.cat([g[1] for g in got])), names


@pytest.fixture(scope='module')
def eval_world_64():
    return _EvalWorld(64)


@pytest.mark.parametrize('scorer', ['fp32', 'fp16_fused', 'fp32_fused'])
def test_acf_evaluation_lists_against_float64(eval_world_64, scorer):
    """embedding_dim = 64 (the fused routes take the first entry of the item tuple through fused_score_transform), 2,000 users x 3,000
    items: the top-20 lists of every route against the float64 scores' ranking with the near-tie acceptance of
    tests/scorer_truth_util.py; the fused routes really call a fused scorer entry point."""
    w = eval_world_64
    got, names = w.lists(scorer)
    assert any(n.startswith('sbr_score_topk_f') for n in names) == (scorer != 'fp32'), names
    assert 'sbr_anchor_mix_fwd' in names
    mag = (w.u64.abs() @ w.i64.abs().t()).to(DEV)
    T.check_against_truth(got, torch.arange(2000, device=DEV), w.masked, ROUTE_C[scorer] * 2.0 ** -24 * mag, 20, what=scorer)


def test_acf_default_width_takes_the_fp32_route():
    w = _EvalWorld(100)
    for scorer in ('fp16_fused', 'fp32_fused'):
        got, names = w.lists(scorer)
        assert not any(n.startswith('sbr_score_topk_f') for n in names), names
        mag = (w.u64.abs() @ w.i64.abs().t()).to(DEV)
        T.check_against_truth(got, torch.arange(2000, device=DEV), w.masked, ROUTE_C['fp32'] * 2.0 ** -24 * mag, 20, what=scorer)


# ---- 8. end to end ------------------------------------------------------------------------------------------------------------------------
def test_acf_fit_end_to_end(tmp_path):
    Sm = S()
    torch.manual_seed(0)
    np.random.seed(0)
    ds = Sm.SyntheticDataset(500, 300, 15000, seed=2, n_negative_samples=4, holdout_per_user=1)
    conf_m = dict(embedding_dim=48, n_anchors=12, delta_exc=0.1, delta_inc=0.01)
    net = Sm.ALGORITHMS['acf'].build_from_conf(conf_m, ds)
    loader = Sm.NegativeSamplingDataLoader(ds, batch_size=256, shuffle=True)
    val = type('L', (), {'dataset': ds.eval_view(), 'batch_size': 256})()
    conf = {'learn': {'lr': 1e-3, 'wd': 0., 'optimizer': 'adam', 'n_epochs': 2}, 'run_settings': {'device': DEV},
            'eval': Sm.evaluation._Cfg(top_k=(10,)), 'results_path': str(tmp_path)}
    tr = Sm.Trainer(net, loader, val, _loss('bce', 300, 4), conf)
    best = tr.fit()
    for k in ('avg_pairwise_proto_sim', 'entity_to_proto_mean', 'entity_to_proto_max', 'entity_to_proto_min'):
        assert k in best and isinstance(best[k], float) and -1.0 <= best[k] <= 1.0, (k, best.get(k))
    assert np.isfinite(best['ndcg@10']) and 0.0 <= best['ndcg@10'] <= 1.0
    losses = tr.train()
    assert list(losses) == ['train/loss', 'train/rec_loss', 'train/reg_loss', 'train/exc_loss', 'train/inc_loss']
    assert all(np.isfinite(v) for v in losses.values()) and losses['train/exc_loss'] > 0
