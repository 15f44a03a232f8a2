"""DeepMatrixFactorization without a GPU: the restatement tests/deepmf_ref.py against the G17 fixture of the real reference (fp32 and
float64, the 1e-5 bound of test_oracle_f64.py), the registry, the configuration keys, the state_dict layout, the legacy checkpoint
mapping, the C ABI additions, and the no-CPU-fallback contract."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import deepmf_ref
from golden_util import GOLDEN, close, host_dataset, load, state_dict, sub, world
from oracle import losses_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(GOLDEN, 'g17_deepmf.json')))['cases']
NEW_SYMBOLS = ('sbr_score_cos_fwd', 'sbr_score_cos_bwd', 'sbr_floor_scores')


def _ref_loss(kind):
    return losses_ref.RefRecLoss(kind, n_items=40, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=3)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_restatement_equals_g17(case, dtype):
    """logits, both losses, every gradient under each loss, all-pairs scores and the floored fraction of every recorded case."""
    z = load('g17_deepmf')
    w = world(z)
    name = case['name']
    mu, kw = deepmf_ref.split_kwargs(case['kwargs'])
    u, i, labels = z['u'], z['i'], torch.from_numpy(z['labels'])
    for kind in ('bce', 'bpr'):
        sd = {k: v.to(dtype).requires_grad_(True) for k, v in state_dict(z, f'{name}/sd/').items()}
        logits = deepmf_ref.forward(sd, w['inter'], w['inter_t'], u, i, mu=mu, **kw)
        close(logits.detach(), z[f'{name}/logits'], what='logits', rtol=1e-5, atol=1e-6)
        loss = _ref_loss(kind).compute_loss(logits, labels)
        close(loss.detach(), z[f'{name}/loss_{kind}'], what=f'{kind} loss', rtol=1e-5, atol=1e-6)
        loss.backward()
        for k, g in sub(z, f'{name}/grad_{kind}/').items():
            close(sd[k].grad, g, what=f'{kind} grad {k}', rtol=1e-5, atol=1e-7, norm_rtol=1e-5)
    floored = float((logits.detach() == mu).double().mean())
    assert floored == case['floored_fraction']
    with torch.no_grad():
        sd = {k: v.to(dtype) for k, v in state_dict(z, f'{name}/sd/').items()}
        close(deepmf_ref.scores_all(sd, w['inter'], w['inter_t'], u, mu=mu, **kw), z[f'{name}/scores_all'], what='all-pairs scores',
              rtol=1e-5, atol=1e-6)


def test_fixture_exercises_the_floor_where_it_says():
    by = {c['name']: c for c in CASES}
    assert by['a_nomid']['floored_fraction'] == 0.0
    assert 0.0 < by['d_norm_repr_floor']['floored_fraction'] < 1.0
    assert len(CASES) >= 5


def test_dmf_is_registered():
    import sibrar_amd as S
    assert S.ALGORITHMS['dmf'] is S.DeepMatrixFactorization
    assert issubclass(S.DeepMatrixFactorization, S.SGDBasedRecommenderAlgorithm)


def test_build_from_conf_parses_the_reference_keys_and_defaults():
    import sibrar_amd as S
    ds = host_dataset(world(load('g17_deepmf')))
    m = S.ALGORITHMS['dmf'].build_from_conf({'final_dimension': 8}, ds)
    assert (m.u_layers, m.i_layers, m.mu) == ([40, 8], [50, 8], 1e-6)
    assert not m.normalize_interactions and not m.normalize_representations and m.user_nn.output_fn is None
    m = S.DeepMatrixFactorization.build_from_conf(dict(u_mid_layers=16, i_mid_layers=[9, 7], final_dimension=6, mu=0.01, normalize_interactions=True,
                                                       normalize_representations=True, use_output_activation_fn=True), ds)
    assert (m.u_layers, m.i_layers, m.mu) == ([40, 16, 6], [50, 9, 7, 6], 0.01)
    assert m.normalize_interactions and m.normalize_representations and isinstance(m.item_nn.output_fn, torch.nn.ReLU)
    with pytest.raises(KeyError):
        S.DeepMatrixFactorization.build_from_conf({}, ds)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_state_dict_keys_and_layout(case):
    import sibrar_amd as S
    z = load('g17_deepmf')
    m = S.DeepMatrixFactorization.build_from_conf(case['kwargs'], host_dataset(world(z)))
    sd = state_dict(z, f'{case["name"]}/sd/')
    assert list(m.state_dict().keys()) == case['keys'] == list(sd.keys())
    m.load_state_dict(sd, strict=True)
    for tower in (m.user_nn, m.item_nn):
        w0 = tower.layers.linear_0.weight
        assert w0.t().is_contiguous() and tuple(w0.shape) == tuple(sd['user_nn.layers.linear_0.weight' if tower is m.user_nn
                                                                     else 'item_nn.layers.linear_0.weight'].shape)
    # general_weight_init: zero biases (train/utils.py:5-13)
    fresh = S.DeepMatrixFactorization.build_from_conf(case['kwargs'], host_dataset(world(z)))
    assert all(float(p.detach().abs().max()) == 0 for k, p in fresh.named_parameters() if k.endswith('bias'))


def test_normalize_interactions_is_folded_into_the_csr_values():
    import sibrar_amd as S
    w = world(load('g17_deepmf'))
    m = S.DeepMatrixFactorization(host_dataset(w), [], [], 4, normalize_interactions=True)
    for rows, mat in ((m._user_rows, w['inter']), (m._item_rows, w['inter_t'])):
        dense = torch.from_numpy(np.asarray(mat.todense())).float()
        ref = dense / torch.linalg.vector_norm(dense, dim=-1, keepdim=True).clamp(min=1e-8)       # sgd_alg.py:1212-1213
        got = torch.zeros_like(dense)
        counts = (rows.indptr[1:] - rows.indptr[:-1])
        got[torch.repeat_interleave(torch.arange(dense.shape[0]), counts), rows.indices.long()] = rows.data
        assert torch.equal(got, ref)


def test_legacy_checkpoint_mapping(tmp_path):
    import sibrar_amd as S
    z = load('g17_deepmf')
    case = next(c for c in CASES if c['name'] == 'b_mid_outact')
    sd = state_dict(z, 'b_mid_outact/sd/')
    legacy = {'user_vectors.weight': torch.zeros(50, 40), 'item_vectors.weight': torch.zeros(40, 50)}
    for k, v in sd.items():
        m = re.match(r'^(\w+)\.layers\.linear_(\d+)\.(\w+)$', k)
        legacy[f'{m[1]}.{2 * int(m[2])}.{m[3]}'] = v
    mapped = S.DeepMatrixFactorization.map_legacy_state_dict(legacy)
    assert list(mapped.keys()) == list(sd.keys()) and all(torch.equal(mapped[k], sd[k]) for k in sd)
    assert S.DeepMatrixFactorization.map_legacy_state_dict(sd) is sd            # a current checkpoint passes through
    torch.save(legacy, tmp_path / 'model.pth')
    net = S.DeepMatrixFactorization.build_from_conf(case['kwargs'], host_dataset(world(z)))
    net.load_model_from_path(str(tmp_path))
    assert all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())
    odd = dict(legacy)
    odd['user_nn.1.weight'] = torch.zeros(1)
    with pytest.raises(ValueError, match='odd layer number'):
        S.DeepMatrixFactorization.map_legacy_state_dict(odd)


def test_new_symbols_declared_and_exported():
    import sibrar_amd as S
    from importlib import import_module
    protos = import_module(S.ops.__name__.rsplit('.', 1)[0] + '._lib').parse_header()
    handle = ctypes.CDLL(S.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in protos, f'{name} is not declared in include/sibrar_hip.h'
        assert hasattr(handle, name), f'{name} is not exported by the library'
    assert len(protos['sbr_score_cos_fwd'][1]) == 12 and len(protos['sbr_score_cos_bwd'][1]) == 13
    assert S.lib().sbr_abi_version() == 4
    header = open(os.path.join(ROOT, 'include', 'sibrar_hip.h')).read()
    assert 'sgd_alg.py:1238-1242' in header


def test_cpu_tensors_raise():
    import sibrar_amd as S
    m = S.DeepMatrixFactorization(host_dataset(world(load('g17_deepmf'))), [], [], 4)
    with pytest.raises(RuntimeError, match='CUDA'):
        m(torch.zeros(2, dtype=torch.long), torch.zeros(2, 3, dtype=torch.long))
    u, i = torch.randn(2, 4), torch.randn(2, 3, 4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.ops.ScoreCosFn.apply(u, i, 1e-6)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.ops.score_cos_all(u, i[0], 1e-6)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.ops.floor_scores_(torch.randn(2, 3), 0.0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.ops.L2NormalizeFn.apply(u, 1e-8)
