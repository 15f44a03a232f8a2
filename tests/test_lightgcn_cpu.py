"""LightGCN without a GPU: the fp32 restatement of sbr_graph_propagate_f32 against float64 inside the derived bound on the worlds the GPU
tests use (tests/lightgcn_ref.py), the symmetry that makes the kernel its own backward pass, L = 0 as plain matrix factorisation, the
registry, build_from_conf and state_dict keys, and the entry's declaration and export."""
import ctypes
import glob
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lightgcn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = os.path.dirname(glob.glob(os.path.join(ROOT, '*', '_lib.py'))[0])
ENTRY = 'sbr_graph_propagate_f32'


def S():
    import sibrar_amd
    return sibrar_amd


@pytest.mark.parametrize('n_users', R.USERS)
@pytest.mark.parametrize('n_items', R.ITEMS)
def test_the_restatement_lies_inside_the_bound_of_float64(n_users, n_items):
    g = R.world(n_users, n_items)
    for d in (3, 64):
        x, s0 = R.table(g.n, d, 1), R.table(g.n, d, 2)
        y, s1 = R.propagate32(g, x, s0, 0.25)
        y64 = R.propagate64(g, x)
        by, bs = R.propagate_bound(g, x, s0, 0.25)
        assert bool((np.abs(y.astype(np.float64) - y64) <= by).all())
        assert bool((np.abs(s1.astype(np.float64) - (s0.astype(np.float64) + y64) * 0.25) <= bs).all())
        assert bool((y[g.deg == 0] == 0).all()) and not bool(np.signbit(y[g.deg == 0]).any())
        # the bound is of the size of the error, not a blanket: some element uses more than a hundredth of it
        if g.m.nnz > 20:
            assert float((np.abs(y - y64) / np.maximum(by, 1e-300)).max()) > 0.01


def test_the_layer_mean_lies_inside_its_bound_and_is_exact_on_the_exact_worlds():
    g = R.world(257, 130)
    e0 = R.table(g.n, 8, 3)
    for n_layers in (1, 3):
        err = np.abs(R.mean32(g, e0, n_layers).astype(np.float64) - R.mean64(g, e0, n_layers))
        assert bool((err <= R.mean_bound(g, e0, n_layers)).all())
    for with_empty in (False, True):
        ge = R.exact_world(0, with_empty)
        ei = R.int_table(ge.n, 5, 4)
        y, s1 = R.propagate32(ge, ei, ei, 1.0)
        assert bool((y.astype(np.float64) == R.propagate64(ge, ei)).all()) and bool((s1.astype(np.float64) == ei + R.propagate64(ge, ei)).all())
        for n_layers in (1, 3):
            assert bool((R.mean32(ge, ei, n_layers).astype(np.float64) == R.mean64(ge, ei, n_layers)).all())


def test_fma32_has_no_double_rounding():
    """(1 + 2^-12)^2 + 2^-60 = 1 + 2^-11 + 2^-24 + 2^-60 lies just above the midpoint of two fp32 neighbours: fmaf rounds up. A float64
    sum rounded to nearest first loses the 2^-60, lands on the midpoint and then goes to the even neighbour, below."""
    a, c = np.float32(1.0 + 2.0 ** -12), np.float32(2.0 ** -60)
    assert float(R.fma32(a, a, c).reshape(-1)[0]) == 1.0 + 2.0 ** -11 + 2.0 ** -23
    assert float(np.float32(np.float64(a) * np.float64(a) + np.float64(c))) == 1.0 + 2.0 ** -11
    assert float(R.fma32(a, a, -c).reshape(-1)[0]) == 1.0 + 2.0 ** -11
    rng = np.random.default_rng(0)
    x, y, z = (rng.standard_normal(1000).astype(np.float32) for _ in range(3))
    assert bool((R.fma32(x, y, np.float32(0)) == (x.astype(np.float64) * y).astype(np.float32)).all())
    assert bool((R.fma32(x, np.float32(1), z) == x + z).all())


def test_the_operator_is_symmetric():
    g = R.world(257, 64)
    rng = np.random.default_rng(0)
    x, z = rng.standard_normal((g.n, 5)), rng.standard_normal((g.n, 5))
    a = g.a_hat()
    assert bool((a == a.T).all())
    lhs, rhs = float(((a @ x) * z).sum()), float((x * (a @ z)).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((np.abs(a) @ np.abs(x) * np.abs(z)).sum())
    for n_layers in (1, 3):
        lhs, rhs = float((R.mean64(g, x, n_layers) * z).sum()), float((x * R.mean64(g, z, n_layers)).sum())
        assert abs(lhs - rhs) <= 1e-12 * (np.abs(x).sum() + np.abs(z).sum())


def test_zero_layers_is_plain_matrix_factorisation():
    g, uw, iw, u, i, labels = R.model_world(8)
    out = R.model_torch(g, uw, iw, u, i, labels, 0, torch.float64)
    plain = (torch.from_numpy(uw).double()[torch.from_numpy(u)][:, None, :] * torch.from_numpy(iw).double()[torch.from_numpy(i)]).sum(-1)
    assert torch.equal(out['logits'], plain)
    assert bool((R.mean32(g, np.concatenate([uw, iw]), 0) == np.concatenate([uw, iw])).all())


def test_registry_conf_and_state_dict_keys():
    Sm = S()
    assert Sm.ALGORITHMS['lightgcn'] is Sm.LightGCN and issubclass(Sm.LightGCN, Sm.SGDBasedRecommenderAlgorithm)
    g = R.world(5, 64)
    ds = SimpleNamespace(n_users=5, n_items=64, user_sampling_matrix_train=g.m)
    net = Sm.ALGORITHMS['lightgcn'].build_from_conf({'embedding_dim': 12, 'n_layers': 2}, ds)
    assert (net.embedding_dim, net.n_layers, net.n_users, net.n_items) == (12, 2, 5, 64)
    default = Sm.LightGCN.build_from_conf({}, ds)
    assert (default.embedding_dim, default.n_layers) == (64, 3)
    assert list(net.state_dict().keys()) == ['user_embeddings.weight', 'item_embeddings.weight']
    assert tuple(net.user_embeddings.weight.shape) == (5, 12) and tuple(net.item_embeddings.weight.shape) == (64, 12)
    # SGDMatrixFactorization's layout: an mf checkpoint without biases loads
    torch.manual_seed(0)
    mf = Sm.SGDMatrixFactorization(5, 64, 12)
    net.load_state_dict(mf.state_dict())
    assert torch.equal(net.user_embeddings.weight, mf.user_embeddings.weight)
    # general_weight_init: N(0, 0.1 / dim)
    big = Sm.LightGCN(5, 64, g.m, embedding_dim=256, n_layers=1)
    assert float(big.item_embeddings.weight.detach().std()) < 3 * 0.1 / 256
    # the matrix is resident, non-persistent and 0/1
    assert tuple(net._graph.shape) == (5, 64) and net._graph.data is None and 'indptr' in dict(net._graph.named_buffers())
    weighted = g.m.copy()
    weighted.data[:] = 2.0
    with pytest.raises(ValueError, match='0/1'):
        Sm.LightGCN(5, 64, weighted)
    with pytest.raises(ValueError, match='training matrix'):
        Sm.LightGCN(6, 64, g.m)
    with pytest.raises(ValueError, match='embedding_dim'):
        Sm.LightGCN(5, 64, g.m, embedding_dim=513)
    with pytest.raises(ValueError, match='n_layers'):
        Sm.LightGCN(5, 64, g.m, n_layers=-1)
    with pytest.raises(RuntimeError, match='CUDA'):
        net(torch.zeros(2, dtype=torch.long), torch.zeros(2, 3, dtype=torch.long))


def test_the_header_declares_the_entry_without_a_leading_dimension():
    text = open(os.path.join(ROOT, 'include', 'sibrar_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    found = re.findall(r'\b' + ENTRY + r'\s*\(([^)]*)\)', text)
    assert len(found) == 1
    params = [' '.join(p.split()) for p in found[0].split(',')]
    assert params == ['const long* u_indptr', 'const int* u_indices', 'const long* i_indptr', 'const int* i_indices', 'int n_users',
                      'int n_items', 'long r0', 'long r1', 'const float* x', 'float* y', 'float* sum', 'float sum_scale', 'int D', 'void* stream']
    assert not any(re.fullmatch(r'(?:const\s+)?long\s+ld\w*', p) for p in params)
    assert 'graph_prop.hip' in open(os.path.join(PACKAGE, 'csrc', 'Makefile')).read()


def test_the_built_library_exports_the_entry():
    from importlib import import_module
    L = import_module(os.path.basename(PACKAGE) + '._lib')
    handle = L.lib()
    assert handle.sbr_abi_version() == 4
    fn = getattr(handle, ENTRY)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 14
    assert fn.argtypes[11] is ctypes.c_float and fn.argtypes[6] is ctypes.c_long and fn.argtypes[4] is ctypes.c_int
