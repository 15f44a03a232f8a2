"""ProtoMF (uprotomf, iprotomf, uiprotomf) without a GPU: the restatement tests/protomf_ref.py against the G18 fixture of the real reference
(fp32 and float64, the bounds of test_deepmf_cpu.py), the registry, the configuration keys, the state_dict layout, the C ABI additions,
the construction of the arg-min-safe inputs the GPU tests use, and the no-CPU-fallback contract."""
import ctypes
import json
import os

import pytest
import torch

import protomf_ref
from golden_util import GOLDEN, I, close, host_dataset, load, state_dict, sub, world
from oracle import losses_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(GOLDEN, 'g18_protomf.json')))['cases']
NEW_SYMBOLS = ('sbr_proto_sim_workspace', 'sbr_proto_sim_fwd', 'sbr_proto_sim_bwd')
SIDE_CONF = dict(embedding_dim=12, n_prototypes=5, sim_proto_weight=0.5, sim_batch_weight=0.25)
UI_CONF = dict(embedding_dim=12, u_n_prototypes=5, i_n_prototypes=7, u_sim_proto_weight=0.5, u_sim_batch_weight=0.25,
               i_sim_proto_weight=0.125, i_sim_batch_weight=2.)


def _ref_loss(kind):
    return losses_ref.RefRecLoss(kind, n_items=I, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=3)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_restatement_equals_g18(case, dtype):
    """logits, every loss-dictionary entry, both losses, every gradient of rec_loss + reg_loss under each loss, all-pairs scores and
    post_val of every recorded case."""
    z = load('g18_protomf')
    name, alg, conf = case['name'], case['alg'], case['conf']
    u, i, labels = z['u'], z['i'], torch.from_numpy(z['labels'])
    for kind in ('bce', 'bpr'):
        sd = {k: v.to(dtype).requires_grad_(True) for k, v in state_dict(z, f'{name}/sd/').items()}
        logits, other = protomf_ref.forward(alg, sd, conf, u, i)
        close(logits.detach(), z[f'{name}/logits'], what='logits', rtol=1e-5, atol=1e-6)
        assert list(other) == case['other_keys']
        for k, v in other.items():
            close(v.detach(), z[f'{name}/other_{kind}/{k}'], what=f'{kind} {k}', rtol=1e-5, atol=1e-6)
        loss = _ref_loss(kind).compute_loss(logits, labels)
        close(loss.detach(), z[f'{name}/loss_{kind}'], what=f'{kind} loss', rtol=1e-5, atol=1e-6)
        (loss + other['reg_loss']).backward()
        for k, g in sub(z, f'{name}/grad_{kind}/').items():
            close(sd[k].grad, g, what=f'{kind} grad {k}', rtol=1e-5, atol=1e-7, norm_rtol=1e-5)
    with torch.no_grad():
        sd = {k: v.to(dtype) for k, v in state_dict(z, f'{name}/sd/').items()}
        close(protomf_ref.scores_all(alg, sd, u, I), z[f'{name}/scores_all'], what='all-pairs scores', rtol=1e-5, atol=1e-6)
        pv = protomf_ref.post_val(alg, sd)
    assert list(pv) == list(case['post_val'])
    for k, v in pv.items():
        close(torch.tensor(v), torch.tensor(case['post_val'][k]), what=f'post_val {k}', rtol=1e-5, atol=1e-6)


def test_fixture_covers_what_it_says():
    by = {c['name']: c for c in CASES}
    assert {c['alg'] for c in CASES} == {'uprotomf', 'iprotomf', 'uiprotomf'}
    assert by['c_ui_5_7']['conf']['u_n_prototypes'] != by['c_ui_5_7']['conf']['i_n_prototypes']
    z = load('g18_protomf')
    zero_user = by['g_u_zero_row']['zero_user']
    assert zero_user == int(z['u'][0]) and float(abs(z['g_u_zero_row/sd/user_embed.weight'][zero_user]).max()) == 0.0
    for name in ('d_u_weights', 'e_i_weights'):
        c = by[name]['conf']
        assert len({c['sim_proto_weight'], c['sim_batch_weight'], 1.0}) == 3
    c = by['f_ui_weights']['conf']
    assert len({c[k] for k in c if k.endswith('_weight')} | {1.0}) == 5


def test_protomf_models_are_registered():
    import sibrar_amd as S
    assert S.ALGORITHMS['uprotomf'] is S.UProtoMF and S.ALGORITHMS['iprotomf'] is S.IProtoMF and S.ALGORITHMS['uiprotomf'] is S.UIProtoMF
    for cls in (S.UProtoMF, S.IProtoMF, S.UIProtoMF):
        assert issubclass(cls, S.PrototypeWrapper) and issubclass(cls, S.SGDBasedRecommenderAlgorithm)
    with pytest.raises(NotImplementedError):
        S.PrototypeWrapper().get_item_representations_pre_tune(None)


def test_build_from_conf_keys_defaults_and_names():
    import sibrar_amd as S
    ds = host_dataset(world(load('g18_protomf')))
    for alg, name in (('uprotomf', 'UProtoMF'), ('iprotomf', 'IProtoMF')):
        m = S.ALGORITHMS[alg].build_from_conf(SIDE_CONF, ds)
        assert (m.name, m.embedding_dim, m.n_prototypes, m.sim_proto_weight, m.sim_batch_weight) == (name, 12, 5, 0.5, 0.25)
        assert tuple(m.prototypes.shape) == (5, 12)
        wide, narrow = (m.user_embed, m.item_embed) if alg == 'uprotomf' else (m.item_embed, m.user_embed)
        assert wide.weight.shape[1] == 12 and narrow.weight.shape[1] == 5
        for key in SIDE_CONF:
            with pytest.raises(KeyError):
                S.ALGORITHMS[alg].build_from_conf({k: v for k, v in SIDE_CONF.items() if k != key}, ds)
        d = S.ALGORITHMS[alg](50, 40)                       # the reference's class defaults
        assert (d.embedding_dim, d.n_prototypes, d.sim_proto_weight, d.sim_batch_weight) == (100, 20, 1., 1.)
        # randn * .1 / embedding_dim: a standard deviation of 1e-3 at the defaults
        assert 5e-4 < float(d.prototypes.detach().std()) < 2e-3
    m = S.ALGORITHMS['uiprotomf'].build_from_conf(UI_CONF, ds)
    assert m.name == 'UIProtoMF' and (m.uprotomf.n_prototypes, m.iprotomf.n_prototypes) == (5, 7)
    assert (m.uprotomf.sim_proto_weight, m.uprotomf.sim_batch_weight, m.iprotomf.sim_proto_weight, m.iprotomf.sim_batch_weight) == (0.5, 0.25, 0.125, 2.)
    assert tuple(m.u_to_i_proj.weight.shape) == (7, 12) and tuple(m.i_to_u_proj.weight.shape) == (5, 12)
    assert not hasattr(m.uprotomf, 'item_embed') and not hasattr(m.iprotomf, 'user_embed')
    for key in UI_CONF:
        with pytest.raises(KeyError):
            S.UIProtoMF.build_from_conf({k: v for k, v in UI_CONF.items() if k != key}, ds)
    d = S.UIProtoMF(50, 40)
    assert (d.embedding_dim, d.uprotomf.n_prototypes, d.iprotomf.n_prototypes) == (100, 20, 20)
    for meth in ('get_user_representations_pre_tune', 'get_user_representations_post_tune', 'get_item_representations_pre_tune',
                 'get_item_representations_post_tune', 'post_val', 'get_and_reset_other_loss'):
        assert callable(getattr(d, meth))
    assert d.get_user_representations_post_tune('x') == 'x' and d.get_item_representations_post_tune('y') == 'y'


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_state_dict_keys_and_order(case):
    import sibrar_amd as S
    z = load('g18_protomf')
    m = S.ALGORITHMS[case['alg']].build_from_conf(case['conf'], host_dataset(world(z)))
    sd = state_dict(z, f'{case["name"]}/sd/')
    assert list(m.state_dict().keys()) == case['keys'] == list(sd.keys())
    assert m.name == case['model_name']
    m.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())


def test_other_loss_accumulates_and_resets_without_a_forward():
    import sibrar_amd as S
    m = S.UProtoMF(50, 40, **SIDE_CONF)
    assert m.get_and_reset_other_loss() == {'reg_loss': 0., 'proto_loss': 0., 'batch_loss': 0.}
    m._acc_r_proto, m._acc_r_batch = torch.tensor(2.), torch.tensor(4.)
    out = m.get_and_reset_other_loss()
    assert list(out) == ['reg_loss', 'proto_loss', 'batch_loss'] and [float(v) for v in out.values()] == [2., 1., 1.]
    assert m._acc_r_proto == 0 and m._acc_r_batch == 0
    ui = S.UIProtoMF(50, 40, **UI_CONF)
    assert list(ui.get_and_reset_other_loss()) == ['reg_loss', 'user_proto_loss', 'user_batch_loss', 'item_proto_loss', 'item_batch_loss']


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
    assert 'sgd_alg.py:48-59' in header and 'sgd_alg.py:394-399' in header and 'TIE RULE' in header
    # the workspace sizes are host arithmetic: the reference defaults, and shapes outside the range
    assert S.lib().sbr_proto_sim_workspace(45056, 100, 20, 0) > 0 and S.lib().sbr_proto_sim_workspace(45056, 100, 20, 1) > 0
    for D, P in ((0, 20), (513, 20), (100, 1), (100, 257)):
        assert S.lib().sbr_proto_sim_workspace(64, D, P, 0) == 0


def test_shapes_outside_the_kernel_range_raise_value_error_before_any_launch():
    import sibrar_amd as S
    # the shape is checked before anything else, so the error does not need a device
    for D, P in ((513, 20), (100, 1), (100, 257)):
        with pytest.raises(ValueError, match='n_prototypes'):
            S.ops.proto_sim(torch.zeros(3, D), None, torch.zeros(P, D))
        with pytest.raises(ValueError, match='n_prototypes'):
            S.ops.ProtoSimFn.apply(torch.zeros(3, D), torch.zeros(2, dtype=torch.long), torch.zeros(P, D))
    with pytest.raises(ValueError, match='one width'):
        S.ops.proto_sim(torch.zeros(3, 8), None, torch.zeros(4, 9))


def test_cpu_tensors_raise():
    import sibrar_amd as S
    u, i = torch.zeros(2, dtype=torch.long), torch.zeros(2, 3, dtype=torch.long)
    for m in (S.UProtoMF(50, 40, **SIDE_CONF), S.IProtoMF(50, 40, **SIDE_CONF), S.UIProtoMF(50, 40, **UI_CONF)):
        with pytest.raises(RuntimeError, match='CUDA'):
            m(u, i)
        with pytest.raises(RuntimeError, match='CUDA'):
            m.post_val(0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.ops.ProtoSimFn.apply(torch.randn(5, 4), u, torch.randn(3, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.ops.proto_sim(torch.randn(5, 4), None, torch.randn(3, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.ops.GatherLinearFn.apply(torch.randn(5, 4), u, torch.randn(3, 4))
    side = S.UProtoMF(50, 40, **SIDE_CONF)
    with pytest.raises(RuntimeError, match='compute_reg_losses'):
        side.compute_reg_losses(torch.ones(2, 5))           # a similarity matrix from anywhere else is an error, not a torch path


def test_argmin_safe_inputs_construction():
    """The inputs of the GPU kernel tests: after the redraws every row's and every column's best / runner-up margin is >= 1e-4 in
    float64 (the GPU test asserts the same before it compares), at the test's shapes that are cheap enough here. D = 1 cannot have
    margins — every similarity is exactly 0 or 2 in every precision (tests/protomf_inputs.py) —: there they are exactly 0 or 2."""
    import protomf_inputs
    for R, D, P in ((37, 100, 20), (2048, 64, 128), (4096, 100, 20), (512, 512, 256)):
        table, rows, protos = protomf_inputs.argmin_safe(R, D, P, seed=R + D + P)
        row_m, col_m = protomf_inputs.margins(table[rows.long()].double(), protos.double())
        assert float(row_m.min()) >= protomf_inputs.MARGIN and float(col_m.min()) >= protomf_inputs.MARGIN, (R, D, P)
        assert table.dtype == torch.float32 and rows.dtype == torch.int32 and tuple(protos.shape) == (P, D)
        assert sorted(rows.tolist()) == list(range(R))
    table, rows, protos = protomf_inputs.argmin_safe(3, 1, 2, seed=6)
    row_m, col_m = protomf_inputs.margins(table[rows.long()].double(), protos.double())
    assert protomf_inputs.exact_only(row_m) and protomf_inputs.exact_only(col_m)
