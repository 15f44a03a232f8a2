"""ACF (acf) without a GPU: the restatement tests/acf_ref.py against the G19 fixture of the real reference (fp32 and float64, the bounds of
test_protomf_cpu.py), the registry, the configuration keys, the initialisation, the state_dict layout, the C ABI additions, the
reference's NaN at q_k == 0 and the no-CPU-fallback contract."""
import ctypes
import json
import math
import os

import pytest
import torch

import acf_ref
from golden_util import GOLDEN, I, close, host_dataset, load, state_dict, sub, world
from oracle import losses_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(GOLDEN, 'g19_acf.json')))['cases']
NEW_SYMBOLS = ('sbr_anchor_mix_workspace', 'sbr_anchor_mix_fwd', 'sbr_anchor_mix_bwd')
CONF = dict(embedding_dim=12, n_anchors=5, delta_exc=0.5, delta_inc=0.25)
TOL = dict(rtol=1e-5, atol=1e-6)


def _ref_loss(kind):
    return losses_ref.RefRecLoss(kind, n_items=I, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=3)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_restatement_equals_g19(case, dtype):
    """logits, every loss-dictionary entry, both losses, every gradient of rec_loss + reg_loss under each loss, all-pairs scores, the
    pre_tune / post_tune outputs of both sides and post_val of every recorded case."""
    z = load('g19_acf')
    name, conf = case['name'], case['conf']
    u, i, labels = z['u'], z['i'], torch.from_numpy(z['labels'])
    for kind in ('bce', 'bpr'):
        sd = {k: v.to(dtype).requires_grad_(True) for k, v in state_dict(z, f'{name}/sd/').items()}
        logits, other = acf_ref.forward(sd, conf, u, i)
        close(logits.detach(), z[f'{name}/logits'], what='logits', **TOL)
        assert list(other) == case['other_keys']
        for k, v in other.items():
            close(v.detach(), z[f'{name}/other_{kind}/{k}'], what=f'{kind} {k}', **TOL)
        loss = _ref_loss(kind).compute_loss(logits, labels)
        close(loss.detach(), z[f'{name}/loss_{kind}'], what=f'{kind} loss', **TOL)
        (loss + other['reg_loss']).backward()
        grads = sub(z, f'{name}/grad_{kind}/')
        assert set(grads) == set(sd)
        for k, g in grads.items():
            close(sd[k].grad, g, what=f'{kind} grad {k}', rtol=1e-5, atol=1e-7, norm_rtol=1e-5)
    with torch.no_grad():
        sd = {k: v.to(dtype) for k, v in state_dict(z, f'{name}/sd/').items()}
        close(acf_ref.scores_all(sd, u, I), z[f'{name}/scores_all'], what='all-pairs scores', **TOL)
        for which, idx in (('user', u), ('item', i)):
            c = acf_ref.pre_tune(sd, which, idx)
            close(c, z[f'{name}/{which}_pre_tune'], what=f'{which} pre_tune', **TOL)
            close(acf_ref.post_tune(sd, c), z[f'{name}/{which}_post_tune'], what=f'{which} post_tune', **TOL)
        pv = acf_ref.post_val(sd)
    assert list(pv) == list(case['post_val'])
    for k, v in pv.items():
        close(torch.tensor(v), torch.tensor(case['post_val'][k]), what=f'post_val {k}', **TOL)


def test_fixture_covers_what_it_says():
    by = {c['name']: c['conf'] for c in CASES}
    assert [(c['embedding_dim'], c['n_anchors']) for c in by.values()] == [(12, 5), (10, 7), (9, 4), (6, 2)]
    assert (by['a_default']['delta_exc'], by['a_default']['delta_inc']) == (0.1, 0.01)
    b, c = by['b_weights'], by['c_weights']
    assert len({b['delta_exc'], b['delta_inc'], c['delta_exc'], c['delta_inc'], 0.1, 0.01}) == 6
    assert (by['d_two_anchors']['delta_exc'], by['d_two_anchors']['delta_inc']) == (1., 1.)
    assert all(c['alg'] == 'acf' and c['model_name'] == 'ACF' and c['other_keys'] == ['reg_loss', 'exc_loss', 'inc_loss'] for c in CASES)


def test_acf_is_registered():
    import sibrar_amd as S
    assert S.ALGORITHMS['acf'] is S.ACF
    assert issubclass(S.ACF, S.PrototypeWrapper) and issubclass(S.ACF, S.SGDBasedRecommenderAlgorithm)


def test_build_from_conf_keys_defaults_and_initialisation():
    import sibrar_amd as S
    ds = host_dataset(world(load('g19_acf')))
    m = S.ALGORITHMS['acf'].build_from_conf(CONF, ds)
    assert (m.name, m.embedding_dim, m.n_anchors, m.delta_exc, m.delta_inc) == ('ACF', 12, 5, 0.5, 0.25)
    assert tuple(m.anchors.shape) == (5, 12) and tuple(m.user_embed.weight.shape) == (50, 12) and tuple(m.item_embed.weight.shape) == (40, 12)
    for key in CONF:
        with pytest.raises(KeyError):
            S.ACF.build_from_conf({k: v for k, v in CONF.items() if k != key}, ds)
    torch.manual_seed(0)
    d = S.ACF(500, 400)                                      # the reference's class defaults
    assert (d.embedding_dim, d.n_anchors, d.delta_exc, d.delta_inc) == (100, 20, 0.1, 0.01)
    # N(0, 1) everywhere: not the small initialisation of general_weight_init
    for t in (d.anchors, d.user_embed.weight, d.item_embed.weight):
        assert 0.9 < float(t.detach().std()) < 1.1
    for meth in ('get_user_representations_pre_tune', 'get_user_representations_post_tune', 'get_item_representations_pre_tune',
                 'get_item_representations_post_tune', 'post_val', 'get_and_reset_other_loss', 'fused_score_transform'):
        assert callable(getattr(d, meth))
    items_fn, users_fn, finish_fn = d.fused_score_transform()
    assert users_fn is None and finish_fn is None and items_fn(('a', 'b', None)) == 'a'


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_state_dict_keys_and_order(case):
    import sibrar_amd as S
    z = load('g19_acf')
    m = S.ALGORITHMS['acf'].build_from_conf(case['conf'], host_dataset(world(z)))
    sd = state_dict(z, f'{case["name"]}/sd/')
    assert list(m.state_dict().keys()) == case['keys'] == list(sd.keys()) == ['anchors', 'user_embed.weight', 'item_embed.weight']
    m.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())


def test_other_loss_keys_and_reset_without_a_forward():
    import sibrar_amd as S
    m = S.ACF(50, 40, **CONF)
    assert m.get_and_reset_other_loss() == {'reg_loss': 0., 'exc_loss': 0., 'inc_loss': 0.}
    m._acc_exc, m._acc_inc = torch.tensor(2.), torch.tensor(4.)
    out = m.get_and_reset_other_loss()
    assert list(out) == ['reg_loss', 'exc_loss', 'inc_loss'] and [float(v) for v in out.values()] == [2., 1., 1.]
    assert m._acc_exc == 0 and m._acc_inc == 0


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
    assert 'sgd_alg.py:261-276' in header and 'sgd_alg.py:246-254' in header and 'sgd_alg.py:76-85' in header and 'NaN CONTRACT' in header
    # the workspace sizes are host arithmetic: the reference defaults, and shapes outside the range
    assert S.lib().sbr_anchor_mix_workspace(45056, 100, 20, 0) > 0 and S.lib().sbr_anchor_mix_workspace(45056, 100, 20, 1) > 0
    for D, K in ((0, 20), (513, 20), (100, 1), (100, 257)):
        assert S.lib().sbr_anchor_mix_workspace(64, D, K, 0) == 0 and S.lib().sbr_anchor_mix_workspace(64, D, K, 1) == 0


def test_shapes_outside_the_kernel_range_raise_value_error_before_any_launch():
    import sibrar_amd as S
    idx = torch.zeros(2, dtype=torch.long)
    for D, K in ((513, 20), (100, 1), (100, 257)):            # the shape is checked before anything else: no device needed
        for want in ('r', 'c'):
            with pytest.raises(ValueError, match='n_anchors'):
                S.ops.anchor_mix(torch.zeros(3, D), None, torch.zeros(K, D), want=want)
        for with_losses in (False, True):
            with pytest.raises(ValueError, match='n_anchors'):
                S.ops.AnchorMixFn.apply(torch.zeros(3, D), idx, torch.zeros(K, D), with_losses)
    with pytest.raises(ValueError, match='one width'):
        S.ops.anchor_mix(torch.zeros(3, 8), None, torch.zeros(4, 9))
    with pytest.raises(ValueError, match='want'):
        S.ops.anchor_mix(torch.zeros(3, 8), None, torch.zeros(4, 8), want='s')


def test_cpu_tensors_raise():
    import sibrar_amd as S
    u, i = torch.zeros(2, dtype=torch.long), torch.zeros(2, 3, dtype=torch.long)
    m = S.ACF(50, 40, **CONF)
    with pytest.raises(RuntimeError, match='CUDA'):
        m(u, i)
    for fn, arg in ((m.get_user_representations, u), (m.get_item_representations, i), (m.get_user_representations_pre_tune, u),
                    (m.get_item_representations_pre_tune, i), (m.get_user_representations_post_tune, torch.zeros(2, 5)),
                    (m.get_item_representations_post_tune, torch.zeros(2, 3, 5))):
        with pytest.raises(RuntimeError, match='CUDA'):
            fn(arg)
    with pytest.raises(RuntimeError, match='CUDA'):
        m.post_val(0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.ops.AnchorMixFn.apply(torch.randn(5, 4), u, torch.randn(3, 4), True)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.ops.anchor_mix(torch.randn(5, 4), None, torch.randn(3, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.ops.cosine_sim(torch.randn(5, 4), None, torch.randn(3, 4))


def test_restatement_records_the_reference_nan_at_an_empty_anchor():
    """Four rows, two anchors, logits (200, 0): in fp32 exp(-200) underflows, c = [1, 0] in every row, q = [1, 0] and the reference's
    inc_loss is NaN (0 log 0) while r, c and exc are finite. float64 still holds exp(-200) = 1.4e-87 (q_1 > 0, inc finite = log 2 to
    working precision); it meets the same NaN from logit 800 on, where exp underflows there too."""
    for dtype, logit in ((torch.float32, 200.), (torch.float32, 800.), (torch.float64, 800.)):
        table, anchors = acf_ref.nan_case(dtype, logit)
        r, c, s = acf_ref.mix(table, anchors)
        exc, inc = acf_ref.losses(c, s)
        assert acf_ref.q_of(c).tolist() == [1., 0.], (dtype, logit)
        assert bool(torch.isnan(inc)) and bool(torch.isfinite(exc)) and float(exc) == 0.
        assert bool(torch.isfinite(r).all()) and c.tolist() == [[1., 0.]] * 4
    table, anchors = acf_ref.nan_case(torch.float64, 200.)
    r, c, s = acf_ref.mix(table, anchors)
    exc, inc = acf_ref.losses(c, s)
    assert float(acf_ref.q_of(c)[1]) > 0 and abs(float(inc) - math.log(2)) < 1e-12
