"""The simplified ProtoMF models (uprotomfs, iprotomfs, uiprotomfs) without a GPU: the restatement tests/protomfs_ref.py against the G21
fixture of the real reference (fp32 and float64, the bounds of test_protomf_cpu.py), the registry, the configuration keys, the state_dict
layout, the combine class, the C ABI additions and the no-CPU-fallback contract."""
import ctypes
import json
import os

import pytest
import torch

import protomfs_ref
from golden_util import GOLDEN, I, close, host_dataset, load, state_dict, sub, world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(GOLDEN, 'g21_protomfs.json')))['cases']
NEW_SYMBOLS = ('sbr_proto_score_workspace', 'sbr_proto_score_fwd', 'sbr_proto_score_bwd')
SIDE_CONF = dict(embedding_dim=12, n_prototypes=5)
UI_CONF = dict(embedding_dim=12, u_n_prototypes=5, i_n_prototypes=7)
STATS = ['avg_pairwise_proto_sim', 'entity_to_proto_mean', 'entity_to_proto_max', 'entity_to_proto_min', 'bin_weights_mean',
         'sum_weights_mean']


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_restatement_equals_g21(case, dtype):
    """logits, both losses, every gradient under each loss, all-pairs scores and post_val of every recorded case."""
    z = load('g21_protomfs')
    name, alg = case['name'], case['alg']
    u, i, labels = z['u'], z['i'], torch.from_numpy(z['labels'])
    for kind in ('bce', 'bpr'):
        sd = {k: v.to(dtype).requires_grad_(True) for k, v in state_dict(z, f'{name}/sd/').items()}
        logits = protomfs_ref.forward(alg, sd, u, i)
        close(logits.detach(), z[f'{name}/logits'], what='logits', rtol=1e-5, atol=1e-6)
        loss = protomfs_ref.rec_loss(kind, logits, labels)
        close(loss.detach(), z[f'{name}/loss_{kind}'], what=f'{kind} loss', rtol=1e-5, atol=1e-6)
        loss.backward()
        grads = sub(z, f'{name}/grad_{kind}/')
        assert list(grads) == case['keys']
        for k, g in grads.items():
            close(sd[k].grad, g, what=f'{kind} grad {k}', rtol=1e-5, atol=1e-7, norm_rtol=1e-5)
    with torch.no_grad():
        sd = {k: v.to(dtype) for k, v in state_dict(z, f'{name}/sd/').items()}
        close(protomfs_ref.scores_all(alg, sd, u, I), z[f'{name}/scores_all'], what='all-pairs scores', rtol=1e-5, atol=1e-6)
        pv = protomfs_ref.post_val(alg, sd)
    assert list(pv) == list(case['post_val'])
    for k, v in pv.items():
        close(torch.tensor(v), torch.tensor(case['post_val'][k]), what=f'post_val {k}', rtol=1e-5, atol=1e-6)


def test_fixture_covers_what_it_says():
    by = {c['name']: c for c in CASES}
    assert [c['alg'] for c in CASES[:3]] == ['uprotomfs', 'iprotomfs', 'uiprotomfs']
    assert by['c_ui_5_7']['conf']['u_n_prototypes'] != by['c_ui_5_7']['conf']['i_n_prototypes']
    assert list(by['a_u']['post_val']) == STATS
    assert list(by['c_ui_5_7']['post_val']) == [f'{s}_{k}' for s in ('user', 'item') for k in STATS]
    z = load('g21_protomfs')
    zero_user = by['d_u_zero_row']['zero_user']
    assert zero_user == int(z['u'][0]) and float(abs(z['d_u_zero_row/sd/user_embed.weight'][zero_user]).max()) == 0.0
    for name, key, used in (('e_u_relu_gate', 'item_embed.weight', z['i']), ('f_i_relu_gate', 'user_embed.weight', z['u'])):
        w = z[f'{name}/sd/{key}'][used.reshape(-1)]
        assert (w == 0).any() and (w < 0).any() and (w > 0).any(), f'{name}: the batch does not meet the ReLU gate on every side'


def test_protomfs_models_are_registered_and_exported():
    import sibrar_amd as S
    assert S.ALGORITHMS['uprotomfs'] is S.UProtoMFs and S.ALGORITHMS['iprotomfs'] is S.IProtoMFs
    assert S.ALGORITHMS['uiprotomfs'] is S.UIProtoMFs
    for cls in (S.UProtoMFs, S.IProtoMFs, S.UIProtoMFs):
        assert issubclass(cls, S.SGDBasedRecommenderAlgorithm) and not issubclass(cls, S.PrototypeWrapper)
        assert cls.get_and_reset_other_loss is S.SGDBasedRecommenderAlgorithm.get_and_reset_other_loss
    assert callable(S.UIProtoMFsCombine) and hasattr(S.ops, 'ProtoCosFn') and hasattr(S.ops, 'ProtoScoreFn')


def test_build_from_conf_keys_defaults_names_and_initialisation():
    import sibrar_amd as S
    ds = host_dataset(world(load('g21_protomfs')))
    for alg, name in (('uprotomfs', 'UProtoMFs'), ('iprotomfs', 'IProtoMFs')):
        m = S.ALGORITHMS[alg].build_from_conf(SIDE_CONF, ds)
        assert (m.name, m.embedding_dim, m.n_prototypes) == (name, 12, 5) and tuple(m.prototypes.shape) == (5, 12)
        wide, narrow = (m.user_embed, m.item_embed) if alg == 'uprotomfs' else (m.item_embed, m.user_embed)
        assert wide.weight.shape[1] == 12 and narrow.weight.shape[1] == 5
        for key in SIDE_CONF:
            with pytest.raises(KeyError):
                S.ALGORITHMS[alg].build_from_conf({k: v for k, v in SIDE_CONF.items() if k != key}, ds)
        torch.manual_seed(3)
        d = S.ALGORITHMS[alg](500, 400)                     # the reference's class defaults
        assert (d.embedding_dim, d.n_prototypes) == (100, 20)
        wide, narrow = (d.user_embed, d.item_embed) if alg == 'uprotomfs' else (d.item_embed, d.user_embed)
        # randn * .1 / embedding_dim and general_weight_init: a standard deviation of 1e-3 at the defaults; the weight side is a
        # truncated normal around 0.5 with the same deviation, inside [0, 1]
        assert 5e-4 < float(d.prototypes.detach().std()) < 2e-3 and 5e-4 < float(wide.weight.detach().std()) < 2e-3
        w = narrow.weight.detach()
        assert abs(float(w.mean()) - 0.5) < 1e-3 and 5e-4 < float(w.std()) < 2e-3 and float(w.min()) >= 0. and float(w.max()) <= 1.
    m = S.ALGORITHMS['uiprotomfs'].build_from_conf(UI_CONF, ds)
    assert m.name == 'UIProtoMFs' and (m.uprotomfs.n_prototypes, m.iprotomfs.n_prototypes) == (5, 7)
    assert tuple(m.u_to_i_proj.weight.shape) == (7, 12) and tuple(m.i_to_u_proj.weight.shape) == (5, 12)
    assert not hasattr(m.uprotomfs, 'item_embed') and not hasattr(m.iprotomfs, 'user_embed')
    for key in UI_CONF:
        with pytest.raises(KeyError):
            S.UIProtoMFs.build_from_conf({k: v for k, v in UI_CONF.items() if k != key}, ds)
    d = S.UIProtoMFs(50, 40)
    assert (d.embedding_dim, d.uprotomfs.n_prototypes, d.iprotomfs.n_prototypes) == (100, 20, 20)
    out = d.get_and_reset_other_loss()
    assert list(out) == ['reg_loss'] and float(out['reg_loss']) == 0.


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_state_dict_keys_and_order(case):
    import sibrar_amd as S
    z = load('g21_protomfs')
    m = S.ALGORITHMS[case['alg']].build_from_conf(case['conf'], host_dataset(world(z)))
    sd = state_dict(z, f'{case["name"]}/sd/')
    assert list(m.state_dict().keys()) == case['keys'] == list(sd.keys())
    assert m.name == case['model_name']
    m.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())


def test_combine_class_refuses_path_and_conf():
    import sibrar_amd as S
    c = S.UIProtoMFsCombine(S.UProtoMFs(50, 40, **SIDE_CONF), S.IProtoMFs(50, 40, **SIDE_CONF))
    assert c.name == 'UIProtoMFsCombine' and isinstance(c.uprotomfs, S.UProtoMFs) and isinstance(c.iprotomfs, S.IProtoMFs)
    with pytest.raises(ValueError, match='saved'):
        c.save_model_to_path('anywhere')
    with pytest.raises(ValueError, match='loaded'):
        c.load_model_from_path('anywhere')
    with pytest.raises(ValueError, match='built'):
        S.UIProtoMFsCombine.build_from_conf({}, None)


def test_new_symbols_declared_and_exported():
    import sibrar_amd as S
    from importlib import import_module
    protos = import_module(S.ops.__name__.rsplit('.', 1)[0] + '._lib').parse_header()
    handle = ctypes.CDLL(S.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in protos, f'{name} is not declared in include/sibrar_hip.h'
        assert hasattr(handle, name), f'{name} is not exported by the library'
    assert S.lib().sbr_abi_version() == 4
    header = open(os.path.join(ROOT, 'include', 'sibrar_hip.h')).read()
    assert 'sgd_alg.py:62-73' in header and 'csrc/proto_cos.hip' in header
    # the workspace sizes are host arithmetic: the reference defaults, and shapes outside the range
    for R in (1, 256, 8192, 45056):
        assert S.lib().sbr_proto_score_workspace(R, 100, 20, 0) > 0 and S.lib().sbr_proto_score_workspace(R, 100, 20, 1) > 0
    assert S.lib().sbr_proto_score_workspace(64, 512, 256, 1) > 0 and S.lib().sbr_proto_score_workspace(64, 1, 2, 1) > 0
    for D, P in ((0, 20), (513, 20), (100, 1), (100, 257)):
        assert S.lib().sbr_proto_score_workspace(64, D, P, 0) == 0 and S.lib().sbr_proto_score_workspace(64, D, P, 1) == 0
    assert S.lib().sbr_proto_score_workspace(0, 100, 20, 0) == 0


def test_shape_errors_raise_value_error_before_any_launch():
    import sibrar_amd as S
    idx = torch.zeros(2, dtype=torch.long)
    # the shape is checked before anything else, so the error does not need a device
    for D, P in ((513, 20), (100, 1), (100, 257)):
        with pytest.raises(ValueError, match='n_prototypes'):
            S.ops.ProtoCosFn.apply(torch.zeros(3, D), idx, torch.zeros(P, D))
        with pytest.raises(ValueError, match='n_prototypes'):
            S.ops.ProtoScoreFn.apply(torch.zeros(3, D), idx, torch.zeros(P, D), torch.zeros(4, P), None, 2)
    with pytest.raises(ValueError, match='one width'):
        S.ops.ProtoCosFn.apply(torch.zeros(3, 8), None, torch.zeros(4, 9))
    t, p = torch.zeros(3, 8), torch.zeros(4, 8)
    with pytest.raises(ValueError, match='as wide as'):                   # weights.shape[1] != P
        S.ops.ProtoScoreFn.apply(t, idx, p, torch.zeros(4, 5), None, 2)
    with pytest.raises(ValueError, match='weight rows'):                  # weights.shape[0] != R * fan
        S.ops.ProtoScoreFn.apply(t, idx, p, torch.zeros(5, 4), None, 2)
    with pytest.raises(ValueError, match='weight rows'):                  # widx.numel() != R * fan
        S.ops.ProtoScoreFn.apply(t, idx, p, torch.zeros(9, 4), torch.zeros(3, dtype=torch.long), 2)
    with pytest.raises(ValueError, match='1 <= fan'):
        S.ops.ProtoScoreFn.apply(t, idx, p, torch.zeros(0, 4), None, 0)


def test_cpu_tensors_raise():
    import sibrar_amd as S
    u, i = torch.zeros(2, dtype=torch.long), torch.zeros(2, 3, dtype=torch.long)
    for m in (S.UProtoMFs(50, 40, **SIDE_CONF), S.IProtoMFs(50, 40, **SIDE_CONF), S.UIProtoMFs(50, 40, **UI_CONF)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            m(u, i)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            m.get_user_representations(u)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            m.post_val(0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.ops.ProtoCosFn.apply(torch.randn(5, 4), u, torch.randn(3, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.ops.ProtoScoreFn.apply(torch.randn(5, 4), u, torch.randn(3, 4), torch.randn(6, 3), i.reshape(-1), 3)
