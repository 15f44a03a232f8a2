"""CPU: the C ABI of the fp32-class fused scorer (csrc/score_topk_f32s.hip) parses from the header and is exported by the library, and
``evaluate_recommender_algorithm`` still rejects scorer names it does not know."""
import ctypes
import os
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch


def _lib():
    return import_module('sibrar---single-branch-recommender_amd._lib')


def test_f32s_prototypes_parse_and_are_exported():
    _l = _lib()
    protos = _l.parse_header()
    vp, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert protos['sbr_score_topk_f32s'][1] == [vp, vp, i, l, i, vp, vp, vp, l, i, i, vp, vp, vp, l, vp, l, i, vp]
    assert protos['sbr_score_topk_f32s'][0] is i
    assert protos['sbr_score_topk_f32s_workspace'] == (l, [l, i, i], ['Bu', 'I', 'k'])
    assert protos['sbr_split_f32_to_bf16x3'][1] == [vp, vp, l, vp]
    # same argument list as the fp16 entry, fp32 users and split item planes in its first two places
    assert protos['sbr_score_topk_f32s'][1] == protos['sbr_score_topk_f16'][1]
    assert protos['sbr_score_topk_f32s'][2][2:] == protos['sbr_score_topk_f16'][2][2:]
    if not os.path.exists(_l.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    h = _l.lib()
    for name in ('sbr_score_topk_f32s', 'sbr_score_topk_f32s_workspace', 'sbr_split_f32_to_bf16x3'):
        assert hasattr(h, name), name
    assert h.sbr_abi_version() == 4
    # the workspace is sized for this route alone: candidate buffers + fill counts, growing with the users, not the catalogue
    w1, w2 = h.sbr_score_topk_f32s_workspace(100_000, 50_000, 20), h.sbr_score_topk_f32s_workspace(100_000, 5_000, 20)
    assert w1 == w2 and w1 < h.sbr_score_topk_f16_workspace(100_000, 50_000, 20)


def test_f32s_host_checks_without_a_gpu():
    import sibrar_amd as S
    assert S.ops.score_topk_f32s_supported(128, 20) and S.ops.score_topk_f32s_supported(64, 32)
    assert not S.ops.score_topk_f32s_supported(256, 20) and not S.ops.score_topk_f32s_supported(128, 33)
    assert not S.ops.score_topk_f32s_supported(8, 10)
    with pytest.raises(RuntimeError):
        S.ops.split_bf16x3(torch.zeros(4, 64))


class _CpuAlg(torch.nn.Module):
    def get_item_representations(self, i):
        return torch.zeros(len(i), 64)

    def get_user_representations(self, u):
        return torch.zeros(len(u), 64)


@pytest.mark.parametrize('name', ['fp64', 'fp32-fused', 'FP32_FUSED', 'fused'])
def test_evaluation_rejects_unknown_scorer_names(name):
    import sibrar_amd as S
    n_u, n_i = 6, 9
    view = SimpleNamespace(n_users=n_u, n_items=n_i, items_in_split=np.arange(n_i), users_in_split=np.arange(n_u), n_items_in_split=n_i,
                           n_users_in_split=n_u, user_sampling_matrix=sp.csr_matrix(np.eye(n_u, n_i)),
                           exclude_data=sp.csr_matrix((n_u, n_i), dtype=bool))
    ev = S.FullEvaluator(config=S.evaluation._Cfg(top_k=(1, 5), calculate_std=False), dataset=view)
    loader = SimpleNamespace(dataset=view, batch_size=4)
    with pytest.raises(ValueError, match='unknown scorer'):
        S.evaluate_recommender_algorithm(_CpuAlg(), loader, ev, 'cpu', scorer=name)
