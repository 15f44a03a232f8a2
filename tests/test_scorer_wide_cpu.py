"""CPU: the Python surface of the wide fused lists (k = 33 .. 128): ``fused_max_k`` validation, the support predicate, the Trainer
conf key, ``Gatherer``, the exported names, and the C interface (ABI version, exported symbols, header comments)."""
import os
import pickle
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def S():
    import sibrar_amd
    return sibrar_amd


@pytest.mark.parametrize('bad', [16, 31, 129, 'a', None, 64.0, True])
def test_fused_max_k_outside_32_to_128_is_a_value_error(bad):
    with pytest.raises(ValueError, match='fused_max_k'):
        S().ops.check_fused_max_k(bad)
    # before anything else is looked at: no dataset, no model, no device needed
    with pytest.raises(ValueError, match='fused_max_k'):
        S().evaluate_recommender_algorithm(None, None, None, 'cpu', fused_max_k=bad)
    with pytest.raises(ValueError, match='fused_max_k'):
        S().gather_recommender_algorithm_results(None, None, None, fused_max_k=bad)


def test_fused_max_k_accepts_32_to_128():
    assert [S().ops.check_fused_max_k(v) for v in (32, 100, 128, np.int64(64))] == [32, 100, 128, 64]


def test_support_predicates():
    ops = S().ops
    # the old predicate keeps its meaning
    assert ops.score_topk_f32s_supported(128, 32) and not ops.score_topk_f32s_supported(128, 33)
    f = ops.score_topk_fused_supported
    for route, dims in (('fp16_fused', (64, 128, 256)), ('fp32_fused', (64, 128))):
        for D in (8, 64, 128, 256):
            assert f(route, D, 32) == (D in dims)
            assert not f(route, D, 33) and not f(route, D, 100)                # default limit: 32
            assert f(route, D, 100, 128) == (D in dims) and f(route, D, 128, max_k=128) == (D in dims)
            assert not f(route, D, 129, 128) and not f(route, D, 0, 128) and not f(route, D, 101, 100)
    assert all(f('fp32_fused', D, k) == ops.score_topk_f32s_supported(D, k) for D in (32, 64, 128, 256) for k in (0, 1, 32, 33))
    with pytest.raises(ValueError):
        f('fp32', 64, 10)
    with pytest.raises(ValueError, match='fused_max_k'):
        f('fp16_fused', 64, 10, 129)


def test_trainer_reads_fused_max_k(tmp_path, monkeypatch):
    import importlib
    trainer = importlib.import_module('sibrar---single-branch-recommender_amd.trainer')
    # (the optimizer owns device buffers; the conf handling under test does not need one)
    monkeypatch.setattr(trainer, 'FusedOptimizer', lambda model, name, lr, weight_decay: type('O', (), {'name': name})())
    conf = {'learn': {'lr': 1e-3, 'wd': 0., 'optimizer': 'adamw', 'n_epochs': 1, 'optimizing_metric': 'ndcg@10'},
            'run_settings': {'device': 'cpu', 'batch_verbose': False}, 'results_path': str(tmp_path), 'fused_step': False}
    net = torch.nn.Linear(2, 2)

    def make(**kw):
        return S().Trainer(net, None, None, None, dict(conf, **kw))
    assert make().fused_max_k == 32 and make().scorer == 'fp32'
    assert make(scorer='fp32_fused', fused_max_k=128).fused_max_k == 128
    for bad in (16, 129, 'a'):
        with pytest.raises(ValueError, match='fused_max_k'):
            make(fused_max_k=bad)


def test_gatherer_collects_arrays_and_objects(tmp_path):
    g = S().Gatherer()
    g.add('a', np.arange(3))
    g.add('a', torch.arange(3, 5))
    g.add('b', torch.ones(2, 4, requires_grad=True))
    g.add('b', np.zeros((1, 4), dtype=np.float32))
    g.add('k', 7)
    g.add('k', 9)                                            # objects: the last one stays
    g.add('metrics', {'ndcg@10': 0.5})
    out = g.gather()
    assert out['a'].tolist() == [0, 1, 2, 3, 4] and out['b'].shape == (3, 4) and out['k'] == 9 and out['metrics'] == {'ndcg@10': 0.5}
    path = str(tmp_path / 'g.pkl')
    g.export_pkl(path)
    back = pickle.load(open(path, 'rb'))
    assert set(back) == set(out) and np.array_equal(back['a'], out['a']) and np.array_equal(back['b'], out['b']) and back['k'] == 9
    g.reset()
    assert g.gather() == {}


def test_new_names_are_exported():
    import importlib
    pkg = importlib.import_module('sibrar---single-branch-recommender_amd')
    for name in ('Gatherer', 'gather_recommender_algorithm_results'):
        assert getattr(S(), name) is getattr(pkg, name) is getattr(pkg.evaluation, name)
    import inspect
    sig = inspect.signature(S().gather_recommender_algorithm_results)
    assert list(sig.parameters)[:6] == ['alg', 'eval_loader', 'evaluator', 'results_path', 'device', 'verbose']
    assert {'scorer', 'fused_max_k', 'user_chunk'} <= set(sig.parameters) and sig.parameters['fused_max_k'].default == 32
    assert inspect.signature(S().evaluate_recommender_algorithm).parameters['fused_max_k'].default == 32


def test_abi_is_still_4_and_the_header_names_the_wide_lists():
    from importlib import import_module
    _lib = import_module('sibrar---single-branch-recommender_amd._lib')
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    handle = _lib.lib()                                      # raises if a declared symbol is not exported
    assert handle.sbr_abi_version() == 4
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r' T (sbr_\w+)', out))
    assert set(_lib.parse_header()) <= exported
    # the wide kernels are instantiations of their own next to the k <= 32 kernels: D = 64, 128, 256 (fp16) and 64, 128 (fp32-class)
    syms = subprocess.run(['nm', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    wide16 = sorted(set(re.findall(r'_Z\d+score_topk_wide_f16_kernelILi(\d+)E', syms)))
    wide32 = sorted(set(re.findall(r'_Z\d+score_topk_wide_f32s_kernelILi(\d+)E', syms)))
    assert wide16 == ['16', '4', '8'] and wide32 == ['4', '8'], (wide16, wide32)
    header = open(os.path.join(ROOT, 'include', 'sibrar_hip.h')).read()
    assert header.count('1 <= k <= 128') == 2 and 'D in {64, 128, 256}, k <= 32' not in header
    # the workspace queries do not depend on k (tests/test_scorer_f32_cpu.py pins their relations at k <= 32)
    for fn in (handle.sbr_score_topk_f16_workspace, handle.sbr_score_topk_f32s_workspace):
        assert fn(100_000, 50_000, 100) == fn(100_000, 50_000, 20) > 0
