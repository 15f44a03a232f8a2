"""GPU: the model-level paths of deterministic mode that DESIGN.md §9 listed as "take these forms or raise; not pinned by a test".

  * a c3-shaped fused step (CSR interactions + tag bag + dense modality, C = 512) with the mode on at a reduced world: the quantities and
    tolerances of test_hip_pinned.test_c3_step_at_full_shapes_against_the_cpu_oracle, the counter at 0, and two 20-step trainings that
    are ``torch.equal`` in every state tensor, both Adam moments and every loss triple, with and without hipGraph;
  * the autograd module path (no FusedTrainStep: net(u, i) -> loss -> backward) on the c1 fixture and on that c3 world;
  * DeepMF (CSR towers), ProtoMF, ACF, ECF through their modules.
For every module path the outcome is pinned in OUTCOME: None — two backward passes from the same parameters, batch and draws give
``torch.equal`` gradients and the counter of arrival-order launches stays 0 — or the entry point whose "no deterministic form" refusal
the backward pass raises. Nothing else is accepted (different bits, a counter above 0, a refusal that names no entry point)."""
import re

import numpy as np
import pytest
import torch

import test_hip_c1 as C1T
from golden_util import close, gscale
from test_hip_c1 import c1                                              # noqa: F401  (the module-scoped fixture)
from test_hip_deterministic import _assert_same, _train
from test_hip_pinned import c3_step_against_the_cpu_oracle

pytestmark = pytest.mark.gpu
DEV = 'cuda'
REFUSAL = re.compile(r'^(sbr_\w+): no deterministic form')

# path -> None: runs on fixed-order forms; a name: the backward pass raises that entry point's refusal
OUTCOME = {'module_c1': None, 'module_c3': None, 'dmf_64': None, 'dmf_516': 'sbr_scatter_add_rows',
           'uprotomf': None, 'uiprotomf': None, 'acf': None, 'ecf': None}


def S():
    import sibrar_amd
    return sibrar_amd


@pytest.fixture
def det():
    ops = S().ops
    prev = ops.set_deterministic(True)
    ops.nondeterministic_launches(reset=True)
    try:
        yield ops
    finally:
        ops.set_deterministic(prev)


def _two_backward_passes(path, ops, net, sd0, run):
    """``run(net)`` -> the scalar to differentiate. Twice from ``sd0`` -> the gradients of the first pass (OUTCOME[path] is None) after
    asserting the second pass gives the same bits and the counter reads 0; or None after asserting the named refusal."""
    want = OUTCOME[path]
    passes = []
    for _ in range(2):
        net.load_state_dict({k: v.to(DEV) for k, v in sd0.items()})
        net.train()
        net.zero_grad(set_to_none=True)
        try:
            run(net).backward()
        except S().SibrarHipError as e:
            m = REFUSAL.match(str(e))
            assert m, f'{path}: a refusal that names no entry point: {e}'
            assert m.group(1) == want, f'{path}: refused by {m.group(1)}, pinned outcome: {want or "runs fixed-order"}'
            torch.cuda.synchronize()
            return None
        torch.cuda.synchronize()
        passes.append({k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None})
    assert want is None, f'{path}: ran, but {want} is pinned to refuse'
    assert passes[0] and set(passes[0]) == set(passes[1])
    bad = [k for k in passes[0] if not torch.equal(passes[0][k], passes[1][k])]
    assert not bad, f'{path}: gradients differ between two identical backward passes: {bad}'
    assert all(bool(torch.isfinite(g).all()) for g in passes[0].values())
    n = ops.nondeterministic_launches()
    assert n == 0, f'{path}: {n} arrival-order launches with the mode on'
    return passes[0]


# ---- the c3-shaped world ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def c3_small():
    """The reduced c3 world; building it IS the fused-step check: one fused step with the mode on against the CPU oracle with the full-size
    test's tolerances (rtol 5e-4, norm 5e-4, losses 1e-4; set for a deeper net, hence loose here), counter 0."""
    ds = S().SyntheticDataset(600, 900, 20_000, item_dense={'audio': 96}, item_tags={'genres': (37, 5)}, seed=0, n_negative_samples=10)
    cfg = {'shared_common_dim': 128, 'user': {'feature_name': 'user_embedding', 'embedding_dim': -1},
           'item': {'features': [{'feature_name': 'interactions'}, {'feature_name': 'genres'}, {'feature_name': 'audio'}],
                    'single_branch_hidden_layers': [512, 256], 'preference_hidden_layers': [],
                    'common_modality_dim': 512, 'embedding_regularization_type': 'pairwise_single',
                    'regularization_temperature': 0.1, 'regularization_weight': 1e-4}}
    w = c3_step_against_the_cpu_oracle(ds, cfg, deterministic=True)
    assert tuple(w.batch[1].shape) == (256, 11)
    errs = {k: float((w.seen[k].cpu().double() - g.double()).abs().max()) / w.scale for k, g in w.grads.items()}
    worst = max(errs, key=errs.get)
    print(f'c3-small, deterministic fused step: worst gradient error {errs[worst]:.2e} of the gradient scale ({worst})')
    return w


def test_c3_shaped_fused_step_in_deterministic_mode(c3_small):
    names = c3_small.names
    assert 'sbr_csr_project_bwd_gather' in names, names
    assert 'sbr_csr_project_bwd' not in names and 'sbr_bag_mean_bwd' not in names, 'a scatter-form gradient ran with the mode on'


@pytest.mark.parametrize('graph', [True, False])
def test_c3_shaped_training_is_bit_identical(c3_small, det, graph):
    w = c3_small
    np.random.seed(42)
    it = iter(S().NegativeSamplingDataLoader(w.ds, batch_size=256, shuffle=True))
    raw = [next(it) for _ in range(5)]

    def make():
        w.net.load_state_dict({k: v.to(DEV) for k, v in w.sd0.items()})
        w.net.train()
        opt = S().FusedOptimizer(w.net, 'adamw', lr=1e-3, weight_decay=0.)
        return w.net, opt, S().FusedTrainStep(w.net, w.lossf, opt, use_graph=graph)

    probe = make()[2]
    batches = [(u, i, l, probe.draw(u.shape, i.shape)) for u, i, l in raw]           # one recorded draw per batch, shared by both runs
    probe.close()
    runs = [_train(make, batches, 20) for _ in range(2)]
    if graph:
        assert runs[0][4].n_replays >= 10, f'only {runs[0][4].n_replays} of 20 steps were graph replays'
    else:
        assert runs[0][4].n_replays == 0
    _assert_same(runs[0], runs[1], f'c3-small graph={graph}')
    assert det.nondeterministic_launches() == 0


# ---- the autograd module path -------------------------------------------------------------------------------------------------------
def test_module_path_c3(c3_small, det):
    w = c3_small
    u, i, labels = w.batch

    def run(net):
        logits = net(u.to(DEV), i.to(DEV), None, w.mods)
        return w.lossf.compute_loss(logits, labels.to(DEV)) + net.get_and_reset_other_loss()['reg_loss'].sum()

    got = _two_backward_passes('module_c3', det, w.net, w.sd0, run)
    if got is not None:
        assert set(w.grads) <= set(got)
        for k, g in w.grads.items():
            close(got[k].cpu(), g, what=f'module path, grad {k}', rtol=5e-4, atol=1e-6, scale=w.scale, norm_rtol=5e-4)


def test_module_path_c1(c1, det):
    w = c1
    batch = w.batches[0]
    u, i, l, mods = batch

    def run(net):
        logits = net(torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV), None, mods)
        return w.bpr.compute_loss(logits, torch.from_numpy(l).to(DEV)) + net.get_and_reset_other_loss()['reg_loss'].sum()

    got = _two_backward_passes('module_c1', det, w.net, w.sd0, run)
    if got is not None:
        grads = C1T.oracle_step(w, w.sd0, 'truth', batch)[2]
        assert set(got) == set(grads)
        sc = gscale(grads.values())
        for k, g in grads.items():                                      # the element-wise bound of test_c1_step_at_full_shape_against_float64
            close(got[k].double().cpu(), g, what=f'module path, grad {k}', rtol=5e-4, atol=1e-7, scale=sc, norm_rtol=1e-4)


# ---- the other models through their modules ------------------------------------------------------------------------------------------
def _model_world(path):
    Sm = S()
    Sm.ops.set_deterministic(True)
    torch.manual_seed(7)
    np.random.seed(7)
    if path.startswith('dmf'):
        import test_hip_deepmf as T                                     # the small builder of its deterministic training test
        ds = Sm.SyntheticDataset(400, 300, 9000, seed=1, n_negative_samples=3)
        width = int(path.split('_')[1])
        return ds, Sm.DeepMatrixFactorization(ds, [width], [width], 64, normalize_representations=True), T._loss('bce', 300), 64
    if path.endswith('protomf'):
        import test_hip_protomf as T
        ds = Sm.SyntheticDataset(400, 300, 9000, seed=1, n_negative_samples=3)
        return ds, Sm.ALGORITHMS[path].build_from_conf(T.DET_CONFS[path], ds), T._loss('bce', 300), 64
    if path == 'acf':
        import test_hip_acf as T
        ds = Sm.SyntheticDataset(2000, 3000, 60000, seed=1, n_negative_samples=3)
        return ds, Sm.ACF(2000, 3000, 64, 20), T._loss('bpr', 3000), 256
    import test_hip_ecf as T
    ds = T._ecf_world(1000, 1500, 30000, 1, n_negative_samples=3)
    return ds, Sm.ALGORITHMS['ecf'].build_from_conf(dict(embedding_dim=32, n_clusters=16, top_n=5, top_m=5), ds), T._loss('bpr', 1500), 256


@pytest.mark.parametrize('path', ['dmf_64', 'dmf_516', 'uprotomf', 'uiprotomf', 'acf', 'ecf'])
def test_model_module_paths(path, det):
    ds, net, lossf, B = _model_world(path)
    net = net.to(DEV).train()
    sd0 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    u, i, labels = next(iter(S().NegativeSamplingDataLoader(ds, batch_size=B, shuffle=False)))

    def run(net):
        logits = net(u.to(DEV), i.to(DEV))
        other = net.get_and_reset_other_loss() if hasattr(net, 'get_and_reset_other_loss') else {}
        loss = lossf.compute_loss(logits, labels.to(DEV))
        return loss + other['reg_loss'].sum() if 'reg_loss' in other else loss

    got = _two_backward_passes(path, det, net, sd0, run)
    if OUTCOME[path] is not None:                                        # the refused path runs outside the mode
        det.set_deterministic(False)
        net.zero_grad(set_to_none=True)
        run(net).backward()
        assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters() if p.grad is not None)
        det.set_deterministic(True)
    else:
        assert any(bool((g != 0).any()) for g in got.values())
