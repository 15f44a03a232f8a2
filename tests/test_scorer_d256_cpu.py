"""CPU: the Python surface and the C interface of the fp32-class fused scorer for 256-wide representations (``fused_max_d``,
``ops.score_topk_f32s_d256``, ``sbr_score_topk_f32s_d256``): validation, the support predicate with and without the new
argument, the Trainer conf key, the new keyword of the two evaluation functions, exported symbols, header text, workspace query."""
import ctypes
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def S():
    import sibrar_amd
    return sibrar_amd


def _lib():
    _l = importlib.import_module('sibrar---single-branch-recommender_amd._lib')
    if not os.path.exists(_l.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _l


@pytest.mark.parametrize('bad', [0, 64, 127, 129, 192, 255, 257, 512, '256', None, 256.0, True])
def test_fused_max_d_other_than_128_or_256_is_a_value_error(bad):
    with pytest.raises(ValueError, match='fused_max_d'):
        S().ops.check_fused_max_d(bad)
    # before anything else is looked at: no dataset, no model, no device needed
    with pytest.raises(ValueError, match='fused_max_d'):
        S().evaluate_recommender_algorithm(None, None, None, 'cpu', fused_max_d=bad)
    with pytest.raises(ValueError, match='fused_max_d'):
        S().gather_recommender_algorithm_results(None, None, None, fused_max_d=bad)
    with pytest.raises(ValueError, match='fused_max_d'):
        S().ops.score_topk_fused_supported('fp32_fused', 256, 20, 32, bad)


def test_fused_max_d_accepts_128_and_256():
    assert [S().ops.check_fused_max_d(v) for v in (128, 256, np.int64(256))] == [128, 256, 256]


def test_support_predicates_with_and_without_max_d():
    ops = S().ops
    f = ops.score_topk_fused_supported
    # the present call forms give the present answers
    assert not ops.score_topk_f32s_supported(256, 20) and ops.score_topk_f32s_supported(128, 20)
    for route, dims in (('fp16_fused', (64, 128, 256)), ('fp32_fused', (64, 128))):
        for D in (8, 64, 128, 192, 256, 512):
            assert f(route, D, 32) == (D in dims) and f(route, D, 100, 128) == (D in dims) and not f(route, D, 33)
            assert f(route, D, 20, 32, 128) == (D in dims) and f(route, D, 20, max_d=128) == (D in dims)
    assert not f('fp32_fused', 256, 20) and not f('fp32_fused', 256, 20, 32) and not f('fp32_fused', 256, 100, 128)
    # max_d = 256 adds D = 256 to the fp32-class route and nothing else
    for D in (8, 64, 128, 192, 256, 512):
        assert f('fp32_fused', D, 20, max_d=256) == (D in (64, 128, 256))
        assert f('fp16_fused', D, 20, max_d=256) == (D in (64, 128, 256))
    assert f('fp32_fused', 256, 1, 32, 256) and f('fp32_fused', 256, 32, 32, 256) and not f('fp32_fused', 256, 33, 32, 256)
    assert f('fp32_fused', 256, 100, 128, 256) and f('fp32_fused', 256, 128, max_k=128, max_d=256)
    assert not f('fp32_fused', 256, 129, 128, 256) and not f('fp32_fused', 256, 0, 128, 256)
    with pytest.raises(ValueError, match='unknown fused scorer'):
        f('fp32', 256, 10, max_d=256)
    with pytest.raises(ValueError, match='fused_max_k'):
        f('fp32_fused', 256, 10, 129, 256)


def test_host_checks_of_the_new_op_without_a_gpu():
    ops = S().ops
    with pytest.raises(RuntimeError):
        ops.score_topk_f32s_d256(torch.zeros(4, 256), torch.zeros(3, 8, 256, dtype=torch.bfloat16), 5)
    sig = inspect.signature(ops.score_topk_f32s_d256)
    assert list(sig.parameters) == ['u32', 'i_planes', 'k', 'u_idx', 'excl_indptr', 'excl_indices', 'item_offset', 'exclusions']
    assert list(sig.parameters) == list(inspect.signature(ops.score_topk_f32s).parameters)


def test_trainer_reads_and_validates_fused_max_d(tmp_path, monkeypatch):
    trainer = importlib.import_module('sibrar---single-branch-recommender_amd.trainer')
    # (the optimizer owns device buffers; the conf handling under test does not need one)
    monkeypatch.setattr(trainer, 'FusedOptimizer', lambda model, name, lr, weight_decay: type('O', (), {'name': name})())
    conf = {'learn': {'lr': 1e-3, 'wd': 0., 'optimizer': 'adamw', 'n_epochs': 1, 'optimizing_metric': 'ndcg@10'},
            'run_settings': {'device': 'cpu', 'batch_verbose': False}, 'results_path': str(tmp_path), 'fused_step': False}
    net = torch.nn.Linear(2, 2)

    def make(**kw):
        return S().Trainer(net, None, None, None, dict(conf, **kw))
    assert make().fused_max_d == 128 and make().fused_max_k == 32
    t = make(scorer='fp32_fused', fused_max_d=256, fused_max_k=128)
    assert (t.scorer, t.fused_max_d, t.fused_max_k) == ('fp32_fused', 256, 128)
    for bad in (64, 257, 'a', 256.0):
        with pytest.raises(ValueError, match='fused_max_d'):
            make(fused_max_d=bad)
    # the evaluations of the Trainer hand the key on
    seen = {}
    monkeypatch.setattr(trainer, 'FullEvaluator', lambda **kw: None)
    monkeypatch.setattr(trainer, 'evaluate_recommender_algorithm', lambda *a, **kw: seen.update(kw) or {})
    t._eval_loader(type('L', (), {'dataset': None})(), None)
    assert seen['fused_max_d'] == 256 and seen['fused_max_k'] == 128 and seen['scorer'] == 'fp32_fused'


def test_the_evaluation_functions_take_fused_max_d_with_default_128():
    for fn in (S().evaluate_recommender_algorithm, S().gather_recommender_algorithm_results):
        p = inspect.signature(fn).parameters
        assert p['fused_max_d'].default == 128 and p['fused_max_k'].default == 32
    # the positional order of the older arguments is what it was
    assert list(inspect.signature(S().gather_recommender_algorithm_results).parameters)[:9] == [
        'alg', 'eval_loader', 'evaluator', 'results_path', 'device', 'verbose', 'scorer', 'fused_max_k', 'user_chunk']
    assert list(inspect.signature(S().evaluate_recommender_algorithm).parameters)[:10] == [
        'alg', 'eval_loader', 'evaluator', 'device', 'return_raw', 'verbose', 'scorer', 'user_chunk', 'shard_items', 'fused_max_k']


def test_the_library_exports_and_the_header_declares_the_new_entries():
    _l = _lib()
    protos = _l.parse_header()
    vp, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    # the argument list of sbr_score_topk_f32s
    assert protos['sbr_score_topk_f32s_d256'] == protos['sbr_score_topk_f32s']
    assert protos['sbr_score_topk_f32s_d256'][0] is i
    assert protos['sbr_score_topk_f32s_d256_workspace'] == (l, [l, i, i], ['Bu', 'I', 'k'])
    h = _l.lib()                                             # raises if a declared symbol is not exported
    assert h.sbr_abi_version() == 4
    out = subprocess.run(['nm', '-D', '--defined-only', _l.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r' T (sbr_\w+)', out))
    assert {'sbr_score_topk_f32s_d256', 'sbr_score_topk_f32s_d256_workspace'} <= exported
    # kernels of their own names; the instantiation sets of the older kernels are what they were
    syms = subprocess.run(['nm', _l.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r'_Z\d+score_topk_f32s_d256_kernel', syms) and re.search(r'_Z\d+score_topk_wide_f32s_d256_kernel', syms)
    assert sorted(set(re.findall(r'_Z\d+score_topk_f32s_kernelILi(\d+)E', syms))) == ['4', '8']
    assert sorted(set(re.findall(r'_Z\d+score_topk_wide_f32s_kernelILi(\d+)E', syms))) == ['4', '8']
    header = open(os.path.join(ROOT, 'include', 'sibrar_hip.h')).read()
    m = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int sbr_score_topk_f32s_d256\(', header, flags=re.S)
    assert m and 'eval/eval.py:216-222' in m.group(1) and '256' in m.group(1)


def test_the_d256_workspace_query_is_positive_and_independent_of_k_and_of_the_catalogue():
    h = _lib().lib()
    fn = h.sbr_score_topk_f32s_d256_workspace
    assert fn(100_000, 25_000, 20) == fn(100_000, 25_000, 100) == fn(100_000, 200_000, 128) == fn(100_000, 25_000, 1) > 0
    assert fn(200_000, 25_000, 20) > fn(100_000, 25_000, 20) >= 100_000 * 4096
    # the older query is untouched by the new geometry (three consumer wave slots instead of seven pad fewer rows)
    assert fn(100_000, 25_000, 20) <= h.sbr_score_topk_f32s_workspace(100_000, 25_000, 20)


def test_the_d256_entry_refuses_other_widths_and_lists_before_touching_a_device():
    _l = _lib()
    h = _l.lib()
    for D, k, msg in ((128, 20, 'D=128 not supported'), (64, 20, 'D=64 not supported'), (256, 0, r'outside \[1, 128\]'),
                      (256, 129, r'outside \[1, 128\]')):
        rc = h.sbr_score_topk_f32s_d256(None, None, D, 64, 100, None, None, None, 0, 0, k, None, None, None, 0, None, 0, 1, None)
        assert rc != 0 and re.search(msg, h.sbr_last_error().decode()), (D, k, h.sbr_last_error().decode())
    # and the older entry keeps its message for D = 256
    rc = h.sbr_score_topk_f32s(None, None, 256, 64, 100, None, None, None, 0, 0, 20, None, None, None, 0, None, 0, 1, None)
    assert rc != 0 and 'D=256 not supported (64, 128)' in h.sbr_last_error().decode()
