"""NeuMF without a GPU: the float32 restatement of 'sbr_neumf_score_all' inside the derived bound of tests/neumf_ref.py on every kernel case of
tests/test_hip_neumf_score.py; the registry, the constructor's refusals, build_from_conf, the state_dict keys, load_pretrained's arithmetic on
CPU tensors; the C ABI of the two entries; the condition under which tests/test_hip_neumf.py asks for exactly the float64 top-10 lists."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import neumf_ref as R


def S():
    import sibrar_amd
    return sibrar_amd


@pytest.mark.parametrize('widths', R.TAILS)
@pytest.mark.parametrize('accumulate', [False, True])
def test_float32_restatement_inside_the_bound(widths, accumulate):
    worst = 0.
    for Bu in R.BUS:
        for I in R.IS:
            c = R.kernel_case(Bu, I, widths)
            want, bound = R.truth_and_bound(c, accumulate)
            got = R.mlp_scores(c, torch.float32, accumulate).double()
            assert bool((bound > 0).all())
            ratio = float(((got - want).abs() / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1., (Bu, I, widths, accumulate, ratio)
    print(f'widths {widths}, accumulate {accumulate}: largest float32-on-CPU error / bound {worst:.3f}')


def test_dead_case_is_dead():
    for widths in R.TAILS:
        c = R.kernel_case(65, 130, widths, dead=True)
        assert float(R.mlp_scores(c, torch.float64, False).sub(float(c['c'][0])).abs().max()) == 0.


def test_registry_and_constructor_refusals():
    Sm = S()
    assert 'neumf' in Sm.ALGORITHMS and Sm.ALGORITHMS['neumf'] is Sm.NeuMF
    assert Sm.ops.NEUMF_MAX_H == 64 and Sm.ops.NEUMF_MAX_LAYERS == 4
    for kw in (dict(gmf_dim=-1), dict(mlp_dim=-1), dict(mlp_layers=(65,)), dict(mlp_layers=(8, 0)), dict(mlp_layers=(8,) * 5),
               dict(gmf_dim=0, mlp_layers=()), dict(mlp_dim=0, mlp_layers=(8,))):
        with pytest.raises(ValueError):
            Sm.NeuMF(40, 30, **kw)
    Sm.NeuMF(40, 30, gmf_dim=0)                                   # the paper's MLP
    Sm.NeuMF(40, 30, mlp_layers=())                               # plain GMF
    Sm.NeuMF(40, 30, mlp_layers=(64, 64, 64, 64))                 # the caps themselves


def test_build_from_conf_round_trips_the_keys_and_state_dict_keys():
    Sm = S()
    ds = SimpleNamespace(n_users=40, n_items=30)
    net = Sm.ALGORITHMS['neumf'].build_from_conf({'gmf_dim': 5, 'mlp_dim': 7, 'mlp_layers': [9, 4], 'unrelated': 1}, ds)
    assert (net.n_users, net.n_items, net.gmf_dim, net.mlp_dim, net.mlp_layers) == (40, 30, 5, 7, (9, 4))
    assert sorted(net.state_dict()) == sorted(R.state_keys(5, 7, (9, 4)))      # (torch lists a module's own parameters first)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {
        'gmf_user.weight': (40, 5), 'gmf_item.weight': (30, 5), 'mlp_user.weight': (40, 7), 'mlp_item.weight': (30, 7),
        'mlp_in_user.weight': (9, 7), 'mlp_in_item.weight': (9, 7), 'mlp_in_bias': (9,), 'mlp_tail.0.weight': (4, 9), 'mlp_tail.0.bias': (4,),
        'out_gmf': (5,), 'out_mlp': (4,), 'out_bias': (1,)}
    default = Sm.ALGORITHMS['neumf'].build_from_conf({}, ds)
    assert (default.gmf_dim, default.mlp_dim, default.mlp_layers) == (8, 32, (32, 16, 8))
    assert sorted(default.state_dict()) == sorted(R.state_keys(8, 32, (32, 16, 8)))
    for name, cfg in R.CONFIGS.items():
        assert sorted(Sm.NeuMF(40, 30, **cfg).state_dict()) == sorted(R.state_keys(**cfg)), name
    assert float(default.gmf_user.weight.detach().std()) < 0.02 and float(default.mlp_in_bias.detach().abs().max()) == 0
    assert not default.dot_product_score
    with pytest.raises(RuntimeError, match='not a dot product'):
        default.fused_score_transform()
    gmf = Sm.NeuMF(40, 30, gmf_dim=64, mlp_layers=())
    items_fn, users_fn, finish_fn = gmf.fused_score_transform()
    assert gmf.dot_product_score and items_fn is None and users_fn is None and callable(finish_fn)
    with pytest.raises(RuntimeError, match='CUDA'):
        default(torch.zeros(2, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int64))


@pytest.mark.parametrize('alpha', [0., 0.25, 1.])
def test_load_pretrained_arithmetic(alpha):
    Sm = S()
    load = lambda net, p: net.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()}) and net
    gmf = load(Sm.NeuMF(40, 30, **R.CONFIGS['gmf']), R.params(seed=1, **R.CONFIGS['gmf']))
    mlp = load(Sm.NeuMF(40, 30, **R.CONFIGS['mlp']), R.params(seed=2, **R.CONFIGS['mlp']))
    net = Sm.NeuMF(40, 30, **R.CONFIGS['full']).load_pretrained(gmf, mlp, alpha=alpha)
    sd, g, m = net.state_dict(), gmf.state_dict(), mlp.state_dict()
    for k in sd:
        if not k.startswith('out_'):
            assert torch.equal(sd[k], (g if k.startswith('gmf_') else m)[k]), k
    assert torch.equal(sd['out_gmf'], alpha * g['out_gmf']) and torch.equal(sd['out_mlp'], (1. - alpha) * m['out_mlp'])
    assert torch.equal(sd['out_bias'], alpha * g['out_bias'] + (1. - alpha) * m['out_bias'])
    # y = alpha y_gmf + (1 - alpha) y_mlp in float64 on the loaded parameters
    u, i, _ = R.batch()
    d = lambda s: {k: v.double() for k, v in s.items()}
    y = R.logits(d(sd), u, i)
    want = alpha * R.logits(d(g), u, i) + (1. - alpha) * R.logits(d(m), u, i)
    assert float((y - want).abs().max()) <= 8 * R.U * float(want.abs().max())
    for bad in (dict(gmf_dim=5, mlp_dim=0, mlp_layers=()), None):
        with pytest.raises(ValueError):
            if bad is None:
                net.load_pretrained(gmf, Sm.NeuMF(40, 30, gmf_dim=0, mlp_dim=6, mlp_layers=(8, 5)), alpha)
            else:
                net.load_pretrained(Sm.NeuMF(40, 30, **bad), mlp, alpha)
    with pytest.raises(ValueError):
        net.load_pretrained(gmf, mlp, alpha=1.5)


def test_c_abi_of_the_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'sibrar_hip.h')).read()
    for entry in ('sbr_neumf_score_all', 'sbr_neumf_score_pairs'):
        assert re.search(r'\bint\s+' + entry + r'\s*\(', text), entry
    lib = __import__('importlib').import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')
    protos = lib.parse_header()
    assert protos['sbr_neumf_score_all'][2] == ['A', 'stride_a', 'Bt', 'stride_b', 'tail', 'tail_len', 'n_layers', 'h1', 'h2', 'h3', 'h4',
                                                'out', 'stride_o', 'Bu', 'I', 'accumulate', 'stream']
    assert S().ops.neumf_tail_len((32, 16, 8)) == 32 * 16 + 16 * 8 + 16 + 8 + 8 + 1
    packed = S().ops.neumf_pack_tail([torch.ones(2, 3)], [torch.full((2,), 2.)], torch.full((2,), 3.), torch.full((1,), 4.))
    assert packed.tolist() == [1.] * 6 + [2.] * 2 + [3.] * 2 + [4.]


def test_the_top_k_condition_of_the_evaluation_test_holds_for_every_user():
    ds, view, p, y, e = R.eval_truth(S())
    left_out, lists = R.left_out_users(y, e)
    print(f'users whose top-{R.EVAL_K} list lies within twice the bound of another order: {left_out}')
    assert len(left_out) == 0
    assert bool(torch.isfinite(torch.gather(y, 1, lists)).all()), 'every user has at least k scored items'
