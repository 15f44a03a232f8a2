"""GPU: BASELINE configs[0] ("c1", the ML-1M shape bench.py times: 5,816 users x 3,299 items, 18 genre tags + 768-d text,
C = D = 64, hidden [64], pairwise InfoNCE, BPR, AdamW 1e-3 / 1e-6) at full size against a float64 oracle.

Every comparison runs three references on the same inputs: the float64 oracle (*truth*; tests/test_oracle_f64.py pins it to the
reference's golden vectors) and the fp32 oracle at 16 threads and at 1 thread, whose different reduction orders show how far an
honest fp32 implementation lands from truth. The criterion for a quantity X, per parameter tensor, is

    err(GPU, truth) <= KAPPA * max(err(CPU16, truth), err(CPU1, truth)) + floor

with KAPPA and the floors fixed before measuring. The tests print the measured ratios err(GPU) / max(err(CPU16), err(CPU1)).

  a) one step at B = 256 and 4096: losses, every gradient, the BatchNorm running statistics, the GEMM entry points called;
  b) no systematic gradient bias: the mean signed gradient error over 32 batches at one fixed parameter state;
  c) a 30-step trajectory with the real optimizer, dense and deferred row-wise AdamW; user representations read mid-training;
  d) one real AdamW step against the update rule in float64 applied to the GPU's own gradient, rows outside the batch included.
"""
import importlib
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from golden_util import bn_shadowed_biases, close, gscale
from oracle import losses_ref, model_ref, sampling_ref, train_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KAPPA = 3.0
LR, WD = 1e-3, 1e-6
N_TRAJ, SNAPS, N_BIAS = 30, (1, 3, 10, 30), 32
THREADS = min(16, os.cpu_count() or 1)
F32, F64 = torch.float32, torch.float64

# the GEMM entry points of one fused c1 step, in launch order: a dispatch change at this shape must be noticed, so that these tests
# keep covering the kernels the bench line times. All on the fp32 pipe at N = 64 (no bf16-split kernel). Forward: the text projector
# (split-K at 256 rows, the plain kernel at 4,096), the two shared layers; backward: weight and input gradient of the second shared
# layer, of the first, the projector's weight gradient (k-slab kernel for every weight gradient)
_BWD = ['sbr_gemm_tn_f32_slabs', 'sbr_gemm_f32', 'sbr_gemm_tn_f32_slabs', 'sbr_gemm_f32', 'sbr_gemm_tn_f32_slabs']
GEMMS = {256: ['sbr_gemm_nt_splitk_f32', 'sbr_gemm_f32', 'sbr_gemm_f32'] + _BWD,
         4096: ['sbr_gemm_f32', 'sbr_gemm_f32', 'sbr_gemm_f32'] + _BWD}


def S():
    import sibrar_amd
    return sibrar_amd


def _lib():
    return importlib.import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')


@pytest.fixture(scope='module')
def c1():
    """The world, model and recorded batches of bench.bench_c1 (its first 30 batches are the bench's), plus a cache of the
    oracle runs that several tests share."""
    bench = importlib.import_module('bench')
    C1 = bench.C1
    ds = S().SyntheticDataset(C1['n_users'], C1['n_items'], C1['nnz'], item_dense={'text': 768}, item_tags={'genres': (18, 3)},
                              seed=0, n_negative_samples=C1['n_neg'], negative_sampling_strategy='uniform_recbole',
                              holdout_per_user=1, item_popularity=1.0)
    torch.manual_seed(42)
    np.random.seed(42)
    net = S().SingleBranchNet(S().SingleBranchNetConfig.from_dict(bench.C1_MODEL), ds).to(DEV)
    sd0 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    ut = {'user_embedding': model_ref.RefTable('categorical', np.arange(ds.n_users), n_categories=ds.n_users)}
    it = {k: model_ref.table_from_feature(f) for k, f in ds.item_features.items()}
    orders = {'item_train': net.item_embedding_module.train_modality_order, 'item_eval': net.item_embedding_module.eval_modality_order}
    rloss = losses_ref.RefRecLoss('bpr', n_items=ds.n_items, aggregator='mean', train_neg_strategy='uniform_recbole',
                                  neg_train=ds.n_negative_samples)
    bpr = S().RecBayesianPersonalizedRankingLoss(n_items=ds.n_items, aggregator='mean', train_neg_strategy='uniform_recbole',
                                                 neg_train=ds.n_negative_samples)
    inter = ds.user_sampling_matrix
    positives = [inter.indices[inter.indptr[u]:inter.indptr[u + 1]] for u in range(ds.n_users)]
    coo = ds.interaction_matrix
    # recorded exactly as bench_c1.cpu_run records: batches from the interaction list, negatives by the reference's collate, the
    # modality draws by the oracle entity's own sampler
    sampler = model_ref.RefSingleBranchNet(dict(sd0), bench.C1_MODEL, ut, it, orders=orders).sides['item']
    rng = np.random.default_rng(0)
    np.random.seed(42)

    def record(B):
        sel = rng.integers(0, coo.nnz, size=B)
        u, i, l = sampling_ref.recbole_collate(coo.row[sel], coo.col[sel], ds.n_negative_samples, ds.items_in_split, positives)
        return u, i, l, sampler.sample_modalities(i.shape, True)

    batches = [record(256) for _ in range(N_TRAJ + N_BIAS)]
    big = record(4096)
    order = list(net.item_embedding_module.train_modality_order)
    lut = {m: q for q, m in enumerate(order)}
    w = SimpleNamespace(ds=ds, net=net, sd0=sd0, ut=ut, it=it, orders=orders, rloss=rloss, bpr=bpr, cfg=bench.C1_MODEL,
                        batches=batches, big=big, order=order, lut=lut, cache={})
    yield w
    torch.set_num_threads(THREADS)


# ---- the oracle sides -------------------------------------------------------------------------------------------------------------
def _copy(sd, dtype):
    """``sd`` with every floating-point tensor in ``dtype`` (float32 -> float64 is exact), trainables requiring grad."""
    out = {}
    for k, v in sd.items():
        v = v.detach().clone()
        if v.dtype.is_floating_point:
            v = v.to(dtype)
            if 'running' not in k:
                v.requires_grad_(True)
        out[k] = v
    return out


SIDES = {'truth': (F64, THREADS), 'cpu16': (F32, THREADS), 'cpu1': (F32, 1)}       # side -> (dtype, threads)


def oracle_step(w, sd_src, side, batch):
    """Forward + backward of one batch on a copy of ``sd_src`` -> (rec loss, reg loss, {key: gradient}, state after the forward)."""
    dtype, threads = SIDES[side]
    torch.set_num_threads(threads)
    try:
        sd = _copy(sd_src, dtype)
        ref = model_ref.RefSingleBranchNet(sd, w.cfg, w.ut, w.it, orders=w.orders)
        u, i, l, mods = batch
        logits = ref.forward(torch.from_numpy(u), torch.from_numpy(i), True, None, mods)
        rl = w.rloss.compute_loss(logits, torch.from_numpy(l))
        rr = ref.get_and_reset_other_loss()['reg_loss'].sum()
        (rl + rr).backward()
        grads = {k: v.grad.detach().double() for k, v in sd.items() if v.requires_grad}
        return float(rl), float(rr), grads, {k: v.detach() for k, v in sd.items()}
    finally:
        torch.set_num_threads(THREADS)


def oracle_trajectory(w, side):
    """N_TRAJ training steps (train/trainer.py:204-223, torch AdamW) from sd0 on the recorded batches -> {step: state} (cached)."""
    key = ('traj', side)
    if key not in w.cache:
        dtype, threads = SIDES[side]
        torch.set_num_threads(threads)
        try:
            sd = _copy(w.sd0, dtype)
            ref = model_ref.RefSingleBranchNet(sd, w.cfg, w.ut, w.it, orders=w.orders)
            opt = train_ref.make_optimizer('adamw', [p for p in sd.values() if p.requires_grad], LR, WD)
            snaps = {}
            for s, (u, i, l, mods) in enumerate(w.batches[:N_TRAJ]):
                train_ref.train_step(ref, w.rloss, opt, torch.from_numpy(u), torch.from_numpy(i), torch.from_numpy(l), None, mods)
                if s + 1 in SNAPS:
                    snaps[s + 1] = {k: v.detach().clone() for k, v in sd.items()}
            w.cache[key] = snaps
        finally:
            torch.set_num_threads(THREADS)
    return w.cache[key]


# ---- the GPU side -----------------------------------------------------------------------------------------------------------------
def gpu_batch(w, batch):
    u, i, l, mods = batch
    pos = np.vectorize(w.lut.__getitem__, otypes=[np.int8])(mods).reshape(-1, mods.shape[-1])
    return torch.from_numpy(u), torch.from_numpy(i), torch.from_numpy(l), (None, (pos, w.order))


def gpu_fused(w, sd, record=None):
    """The bench's model loaded with ``sd``, a fresh FusedOptimizer + FusedTrainStep; with ``record`` (a list) the optimizer launch
    is replaced by a recorder of every parameter gradient (parameters stay as they are)."""
    net = w.net
    net.load_state_dict({k: v.to(DEV) for k, v in sd.items()})
    net.train()
    opt = S().FusedOptimizer(net, 'adamw', lr=LR, weight_decay=WD)
    fused = S().FusedTrainStep(net, w.bpr, opt)
    if record is not None:
        def _record(*a, **k):                                  # stands in for the optimizer launch (which also resets the gradient)
            record.append({k_: p.grad.detach().double().cpu() for k_, p in net.named_parameters()})
            if k.get('zero_grad'):
                opt.fp.grad.zero_()
            return False
        opt.step_flat = _record
    return net, opt, fused


def _state(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


# ---- the criterion ------------------------------------------------------------------------------------------------------------------
class Verdict:
    """Collects every comparison (printed, so the ratios can be quoted) and fails once at the end with all offenders listed."""

    def __init__(self, title):
        self.title, self.lines, self.bad = title, [], []

    def kappa(self, what, e_gpu, e16, e1, floor):
        cpu = max(e16, e1)
        ok = e_gpu <= KAPPA * cpu + floor
        line = (f'{what:<72} gpu {e_gpu:.3e}  cpu16 {e16:.3e}  cpu1 {e1:.3e}  ratio {e_gpu / cpu if cpu > 0 else float("inf"):6.2f}'
                f'  floor {floor:.2e}{"" if ok else "  FAIL"}')
        self.lines.append(line)
        if not ok:
            self.bad.append(line)

    def check(self, what, ok, detail=''):
        if not ok:
            self.bad.append(f'{what}: {detail}')
            self.lines.append(f'{what}: FAIL {detail}')

    def done(self):
        print(f'\n==== {self.title} (KAPPA = {KAPPA})')
        print('\n'.join(self.lines))
        assert not self.bad, f'{self.title}: {len(self.bad)} comparison(s) fail:\n' + '\n'.join(self.bad)


def _err(a, b):
    return float((a.double() - b.double()).norm())


# ---- a) one step at full shape ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [256, 4096])
def test_c1_step_at_full_shape_against_float64(c1, B):
    """One fused step (the bench's first recorded batch at 256; one recorded batch of 4,096) against truth and both fp32 runs:
    rec / reg loss (1e-5 relative of truth and the KAPPA criterion), every parameter gradient (KAPPA, floor 1e-7 ||g_truth||, and
    element-wise within 5e-4 of the gradient scale), every BatchNorm running statistic after the step (counter exactly, stats by
    KAPPA with floor 1e-7 relative), and the GEMM entry points the step called."""
    w = c1
    batch = w.batches[0] if B == 256 else w.big
    seen = []
    net, opt, fused = gpu_fused(w, w.sd0, record=seen)
    lib = _lib()
    lib.CALL_LOG = []
    try:
        total, rec, reg = fused.step(*gpu_batch(w, batch))
    finally:
        log, lib.CALL_LOG = lib.CALL_LOG, None
    rec, reg = float(rec), float(reg)
    after = _state(net)
    fused.close()
    assert len(seen) == 1
    ref = {s: oracle_step(w, w.sd0, s, batch) for s in ('truth', 'cpu16', 'cpu1')}
    v = Verdict(f'c1 one step, B = {B}')
    for q, name in ((0, 'rec loss'), (1, 'reg loss')):
        t = ref['truth'][q]
        got = rec if q == 0 else reg
        v.check(f'{name} within 1e-5 of truth', abs(got - t) <= 1e-5 * abs(t), f'gpu {got!r} truth {t!r}')
        v.kappa(name, abs(got - t), abs(ref['cpu16'][q] - t), abs(ref['cpu1'][q] - t), 1e-7 * abs(t))
    grads = ref['truth'][2]
    shadowed = bn_shadowed_biases(after.keys())
    assert set(grads) == set(seen[0])
    sc = gscale(grads.values())
    for k, g in grads.items():
        # element-wise: what the c2 / c3 tests bound; for a bias in front of a BatchNorm (zero gradient by maths) this is the only bound
        close(seen[0][k], g, what=f'grad {k}', rtol=5e-4, atol=1e-7, scale=sc, norm_rtol=1e-4)
        if k not in shadowed:
            v.kappa(f'grad {k}', _err(seen[0][k], g), _err(ref['cpu16'][2][k], g), _err(ref['cpu1'][2][k], g), 1e-7 * float(g.norm()))
    n_stats = 0
    for k, t in ref['truth'][3].items():
        if 'num_batches_tracked' in k:
            v.check(k, int(after[k]) == int(t) == 1, f'gpu {int(after[k])} truth {int(t)}')
        elif 'running' in k and k not in shadowed:
            n_stats += 1
            v.kappa(k, _err(after[k], t), _err(ref['cpu16'][3][k], t), _err(ref['cpu1'][3][k], t), 1e-7 * float(t.double().norm()))
    assert n_stats >= 1
    gemms = [n_ for n_, _ in log if n_.startswith('sbr_gemm')]
    v.lines.append(f'GEMM entry points: {gemms}')
    v.check('GEMM entry points', gemms == GEMMS[B], f'{gemms} != {GEMMS[B]}')
    v.done()


# ---- b) no systematic gradient bias -------------------------------------------------------------------------------------------------
def test_c1_gradient_has_no_systematic_bias(c1):
    """At one fixed fp32 state theta (truth after 30 steps, rounded to fp32) and 32 recorded batches of 256: per tensor the norm of
    the MEAN signed gradient error (1/N) sum_b (g_side,b - g_truth,b), GPU against both fp32 runs (KAPPA, floor 1e-8 rms_b
    ||g_truth,b||). Rounding noise averages down over the batches, a systematic error (a wrong constant, a dropped term) does not:
    this sees errors far below the element-wise tolerance of a single-batch test."""
    w = c1
    theta = {k: (v.to(F32) if v.dtype.is_floating_point else v) for k, v in oracle_trajectory(w, 'truth')[N_TRAJ].items()}
    batches = w.batches[N_TRAJ:N_TRAJ + N_BIAS]
    seen = []
    net, opt, fused = gpu_fused(w, theta, record=seen)
    for batch in batches:
        fused.step(*gpu_batch(w, batch))
    fused.close()
    assert len(seen) == N_BIAS
    shadowed = bn_shadowed_biases(w.sd0.keys())
    sums = {s: {} for s in ('gpu', 'cpu16', 'cpu1')}
    sq = {}
    for b, batch in enumerate(batches):
        truth = oracle_step(w, theta, 'truth', batch)[2]
        sides = {'gpu': seen[b], 'cpu16': oracle_step(w, theta, 'cpu16', batch)[2], 'cpu1': oracle_step(w, theta, 'cpu1', batch)[2]}
        for k, g in truth.items():
            if k in shadowed:
                continue
            for s, gs in sides.items():
                sums[s][k] = sums[s].get(k, 0.) + (gs[k] - g)
            sq[k] = sq.get(k, 0.) + float(g.norm()) ** 2
    v = Verdict(f'c1 gradient bias over {N_BIAS} batches of 256')
    for k in sq:
        bias = {s: float(sums[s][k].norm()) / N_BIAS for s in sums}
        v.kappa(f'bias {k}', bias['gpu'], bias['cpu16'], bias['cpu1'], 1e-8 * (sq[k] / N_BIAS) ** 0.5)
    v.done()


# ---- c) 30 steps with the real optimizer --------------------------------------------------------------------------------------------
def _rel(a, truth, theta0):
    return float((a.double() - truth.double()).norm() / (truth.double() - theta0.double()).norm().clamp_min(1e-30))


@pytest.mark.parametrize('deferred', ['0', '1'])
def test_c1_30_step_trajectory_against_float64(c1, deferred, monkeypatch):
    """30 real fused steps (dense AdamW launch, or the deferred row-wise AdamW of the user table: c1's default) on the bench's first
    30 recorded batches; after steps 1, 3, 10 and 30 every parameter and BatchNorm statistic against the truth trajectory, as the
    relative distance ||theta_side - theta_truth|| / ||theta_truth - theta_0|| per tensor (KAPPA, floor 2e-6). At step 30 the user
    representations read while the fused step is open (Trainer.val mid-training) equal those read after close(), bit for bit."""
    monkeypatch.setenv('SBR_DEFERRED_ADAM', deferred)
    w = c1
    net, opt, fused = gpu_fused(w, w.sd0)
    assert (fused.deferred is not None) == (deferred == '1')
    snaps = {}
    users = torch.arange(w.ds.n_users, device=DEV)
    for s, batch in enumerate(w.batches[:N_TRAJ]):
        fused.step(*gpu_batch(w, batch))
        if s + 1 == N_TRAJ:
            net.eval()
            with torch.no_grad():
                open_repr = net.get_user_representations(users).clone()
            net.train()
        if s + 1 in SNAPS:
            snaps[s + 1] = _state(net)
    fused.close()
    net.eval()
    with torch.no_grad():
        closed_repr = net.get_user_representations(users).clone()
    net.train()
    refs = {s: oracle_trajectory(w, s) for s in ('truth', 'cpu16', 'cpu1')}
    shadowed = bn_shadowed_biases(w.sd0.keys())
    v = Verdict(f'c1 {N_TRAJ}-step trajectory, SBR_DEFERRED_ADAM = {deferred}')
    v.check('user representations open == closed', torch.equal(open_repr, closed_repr),
            f'max abs diff {float((open_repr - closed_repr).abs().max()):.3e}')
    for t in SNAPS:
        truth = refs['truth'][t]
        for k, x in truth.items():
            if 'num_batches_tracked' in k:
                v.check(f'step {t} {k}', int(snaps[t][k]) == int(x) == t, f'gpu {int(snaps[t][k])} truth {int(x)}')
            elif x.dtype.is_floating_point and k not in shadowed:
                z = w.sd0[k]
                v.kappa(f'step {t:>2} {k}', _rel(snaps[t][k], x, z), _rel(refs['cpu16'][t][k], x, z), _rel(refs['cpu1'][t][k], x, z), 2e-6)
    v.done()


# ---- d) one real AdamW step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('deferred', ['0', '1'])
def test_c1_one_real_adamw_step_against_the_update_rule(c1, deferred, monkeypatch):
    """The optimizer isolated: the GPU's own gradient of the bench's first batch, recorded right before the real optimizer launch,
    through train_ref.adamw_update in float64 must give the parameters (and moments) the launch left — dense launch and deferred
    row-wise table — within a few fp32 ulps of the operands (4e-7 (|p0| + lr)) on every element of every parameter. Rows outside the
    batch included: their step-1 movement (weight decay only, 1e-9 relative) is below one fp32 ulp, so they come out unchanged."""
    monkeypatch.setenv('SBR_DEFERRED_ADAM', deferred)
    w = c1
    net, opt, fused = gpu_fused(w, w.sd0)
    assert (fused.deferred is not None) == (deferred == '1')
    real = opt.step_flat
    got = {}

    def _spy(*a, **k):
        got['g'], got['p0'] = opt.fp.grad.detach().double().cpu(), opt.fp.flat.detach().double().cpu()
        return real(*a, **k)
    opt.step_flat = _spy
    fused.step(*gpu_batch(w, w.batches[0]))
    fused.close()                                              # brings a row-wise updated table up to date
    assert opt.step_count == 1
    fp = opt.fp
    flat, m, vv = fp.flat.detach().double().cpu(), opt.m.detach().double().cpu(), opt.v.detach().double().cpu()
    name_of = {id(p): k for k, p in net.named_parameters()}
    table = 'user_embedding_module.embedding_layer.weight'
    seen_table = False
    for p, o, n in zip(fp.params, fp.offsets, fp.sizes):
        k = name_of[id(p)]
        g, p0 = got['g'][o:o + n], got['p0'][o:o + n]
        want, wm, wv = train_ref.adamw_update(p0, g, torch.zeros_like(g), torch.zeros_like(g), 1, LR, WD)
        for what, a, b, tol in ((k, flat[o:o + n], want, 4e-7 * (p0.abs() + LR)), (f'm of {k}', m[o:o + n], wm, 4e-7 * wm.abs()),
                                (f'v of {k}', vv[o:o + n], wv, 4e-7 * wv.abs())):
            err = (a - b).abs()
            assert bool((err <= tol).all()), f'{what}: max abs err {float(err.max()):.3e}, {int((err > tol).sum())} elements out'
        zero = g == 0
        assert torch.equal(flat[o:o + n][zero], p0[zero]), f'{k}: elements without gradient moved'
        if k == table:
            seen_table = True
            rows = g.view(p.shape).abs().sum(1) > 0
            batch_users = np.unique(w.batches[0][0])
            assert int(rows.sum()) == len(batch_users) and bool(rows[torch.from_numpy(batch_users)].all())
            assert int((~rows).sum()) > 0 and torch.equal(flat[o:o + n].view(p.shape)[~rows], p0.view(p.shape)[~rows])
    assert seen_table
