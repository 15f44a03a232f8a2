"""NGCF without a GPU: the fp32 restatement of sbr_ngcf_layer_fwd against float64 inside the derived bound on the worlds the GPU tests use
(tests/ngcf_ref.py), the backward formulas against float64 autograd, the registry, build_from_conf, state_dict keys and representation
width, an mf checkpoint, the constructor's refusals, and the entries' declaration and export."""
import ctypes
import glob
import os
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lightgcn_ref as L
import ngcf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = os.path.dirname(glob.glob(os.path.join(ROOT, '*', '_lib.py'))[0])
ENTRIES = ('sbr_ngcf_layer_fwd', 'sbr_ngcf_layer_bwd')


def S():
    import sibrar_amd
    return sibrar_amd


@pytest.mark.parametrize('n_items', R.ITEMS)
@pytest.mark.parametrize('n_users', R.USERS)
def test_the_restatement_lies_inside_the_bound_of_float64(n_users, n_items):
    """every world of the GPU test; the nine width pairs go round the nine worlds three at a time, both rates each"""
    k = 3 * R.USERS.index(n_users) + R.ITEMS.index(n_items)
    tight = []
    for din, dout in (R.WIDTHS[(k + j) % 9] for j in (0, 3, 6)):
        for p in R.RATES:
            c = R.case(n_users, n_items, din, dout, p)
            for name in ('z', 'h', 'out'):
                err = np.abs(c['r32'][name].astype(np.float64) - c['r64'][name])
                assert bool((err <= c['bound'][name]).all()), (din, dout, p, name, float((err / np.maximum(c['bound'][name], 1e-300)).max()))
                tight.append(float((err / np.maximum(c['bound'][name], 1e-300)).max()))
            if p > 0:
                assert bool((c['r32']['h'][~c['keep']] == 0).all()) and not bool(np.signbit(c['r32']['h'][~c['keep']]).any())
                frac = float(c['keep'].mean())
                assert c['keep'].size < 200 or abs(frac - (1 - p)) < 0.1, frac
            n = np.sqrt((c['r32']['out'].astype(np.float64) ** 2).sum(1))
            assert bool(((np.abs(n - 1) < 1e-5) | (n == 0)).all())
    # the bound is of the size of the error, not a blanket
    assert max(tight) > 0.01, max(tight)


def test_the_sum_of_squares_order_and_the_mask_are_what_the_header_states():
    rng = np.random.default_rng(0)
    h = rng.standard_normal((5, 70)).astype(np.float32)
    t = [np.float32(0)] * 16
    for j in range(70):                                                       # ascending columns, partial (j / 4) % 16
        t[(j // 4) % 16] = np.float32(t[(j // 4) % 16] + np.float32(h[2, j] * h[2, j]))
    for o in (1, 2, 4, 8):
        t = [np.float32(t[l] + t[l ^ o]) for l in range(16)]
    assert R.sumsq32(h)[2] == t[0]
    assert abs(float(R.sumsq32(h)[2]) - float((h[2].astype(np.float64) ** 2).sum())) < 1e-4
    # the mask is a function of (seed, stream, row, column): rows can be asked for in any split
    whole = R.keep_mask(R.SEED, R.STREAM, np.arange(40), 33, 0.3)
    assert bool((R.keep_mask(R.SEED, R.STREAM, np.arange(17, 29), 33, 0.3) == whole[17:29]).all())
    assert not bool((R.keep_mask(R.SEED, R.STREAM + 1, np.arange(40), 33, 0.3) == whole).all())
    assert bool(R.keep_mask(1, 2, np.arange(3), 4, 0.0).all())
    assert float(R.inv_keep32(0.0)) == 1.0 and R.inv_keep32(0.3).dtype == np.float32


@pytest.mark.parametrize('p', R.RATES)
def test_the_backward_formulas_agree_with_float64_autograd(p):
    g = R.world(63, 64)
    din, dout = 8, 5
    x = L.table(g.n, din, 3)
    W1, W2, bias = R.weights(din, dout)
    rng = np.random.default_rng(5)
    g_out, g_h = rng.standard_normal((g.n, dout)).astype(np.float32), rng.standard_normal((g.n, dout)).astype(np.float32)
    fwd = R.layer32(g, x, W1, W2, bias, R.SLOPE, p, R.SEED, 2)
    keep = None if p == 0 else R.keep_mask(R.SEED, 2, np.arange(g.n), dout, p)
    for gh in (None, g_h):
        ref = R.layer_grads_torch(g, x, W1, W2, bias, R.SLOPE, keep, R.inv_keep32(p), g_out, gh, torch.float64)
        got = R.layer_bwd32(g, x, W1, W2, R.SLOPE, p, R.SEED, 2, fwd['h'], g_out, gh)
        for k in ('dx', 'dW1', 'dW2', 'dbias'):
            err = float(np.abs(got[k].astype(np.float64) - ref[k].numpy()).max())
            assert err <= 1e-4 * max(1.0, float(ref[k].abs().max())), (k, err)


def test_registry_conf_state_dict_keys_and_width():
    Sm = S()
    assert Sm.ALGORITHMS['ngcf'] is Sm.NGCF and issubclass(Sm.NGCF, Sm.LightGCN)
    g = L.world(5, 64)
    ds = SimpleNamespace(n_users=5, n_items=64, user_sampling_matrix_train=g.m)
    net = Sm.ALGORITHMS['ngcf'].build_from_conf({'embedding_dim': 12, 'layer_sizes': [8, 6], 'message_dropout': 0.25, 'leaky_slope': 0.1}, ds)
    assert (net.embedding_dim, net.layer_sizes, net.message_dropout, net.leaky_slope, net.n_layers) == (12, (8, 6), 0.25, 0.1, 2)
    assert net.repr_dim == 12 + 8 + 6
    default = Sm.NGCF.build_from_conf({}, ds)
    assert (default.embedding_dim, default.layer_sizes, default.message_dropout, default.leaky_slope, default.repr_dim) == (64, (64, 64, 64), 0.1, 0.2, 256)
    assert list(net.state_dict().keys()) == ['user_embeddings.weight', 'item_embeddings.weight', 'w_gc.0', 'w_gc.1', 'w_bi.0', 'w_bi.1', 'b.0', 'b.1']
    assert sorted(net.state_dict().keys()) == sorted(R.param_names(2))
    assert tuple(net.w_gc[0].shape) == (12, 8) and tuple(net.w_bi[1].shape) == (8, 6) and tuple(net.b[1].shape) == (6,)
    # Xavier-uniform weights, zero biases, general_weight_init tables
    lim = float(np.sqrt(6.0 / (64 + 64)))
    w = default.w_gc[1].detach()
    assert float(w.abs().max()) <= lim and float(w.std()) > 0.4 * lim and not bool(default.b[0].detach().any())
    assert float(default.item_embeddings.weight.detach().std()) < 3 * 0.1 / 64
    # an mf checkpoint without biases loads
    torch.manual_seed(0)
    mf = Sm.SGDMatrixFactorization(5, 64, 12)
    res = net.load_state_dict(mf.state_dict(), strict=False)
    assert not res.unexpected_keys and sorted(res.missing_keys) == sorted(R.param_names(2)[2:])
    assert torch.equal(net.user_embeddings.weight, mf.user_embeddings.weight)
    plain = Sm.NGCF(5, 64, g.m, embedding_dim=12, layer_sizes=())
    plain.load_state_dict(mf.state_dict())
    assert list(plain.state_dict().keys()) == ['user_embeddings.weight', 'item_embeddings.weight'] and plain.repr_dim == 12
    with pytest.raises(RuntimeError, match='CUDA'):
        net(torch.zeros(2, dtype=torch.long), torch.zeros(2, 3, dtype=torch.long))


def test_constructor_refusals():
    Sm = S()
    g = L.world(5, 64)
    for kw in ({'embedding_dim': 129}, {'layer_sizes': (64, 129)}, {'layer_sizes': (0,)}, {'embedding_dim': 0}):
        with pytest.raises(ValueError, match=r'\[1, 128\]'):
            Sm.NGCF(5, 64, g.m, **kw)
    weighted = g.m.copy()
    weighted.data[:] = 2.0
    with pytest.raises(ValueError, match='0/1'):
        Sm.NGCF(5, 64, weighted)
    with pytest.raises(ValueError, match='training matrix'):
        Sm.NGCF(6, 64, g.m)
    for p in (-0.1, 1.0, 1.5, float('nan')):
        with pytest.raises(ValueError, match='message_dropout'):
            Sm.NGCF(5, 64, g.m, message_dropout=p)
    for s in (0.0, -0.2, 1.5, float('nan')):
        with pytest.raises(ValueError, match='leaky_slope'):
            Sm.NGCF(5, 64, g.m, leaky_slope=s)


def test_the_header_declares_both_entries_and_the_library_exports_them():
    lib = import_module(os.path.basename(PACKAGE) + '._lib')
    protos = lib.parse_header()
    fwd, bwd = (protos[e] for e in ENTRIES)
    assert fwd[2] == ['u_indptr', 'u_indices', 'i_indptr', 'i_indices', 'n_users', 'n_items', 'r0', 'r1', 'x', 'Din', 'W1', 'W2', 'bias', 'Dout',
                      'slope', 'p', 'seed', 'stream_id', 'h', 'out', 'out_ld', 'stream']
    assert fwd[1][14] is ctypes.c_float and fwd[1][16] is ctypes.c_ulong and fwd[1][20] is ctypes.c_long and fwd[1][6] is ctypes.c_long
    assert bwd[2][17:] == ['h', 'g_out', 'out_ld', 'g_h', 'ds', 'dx_direct', 'dW1', 'dW2', 'dbias', 'workspace', 'workspace_bytes', 'stream']
    assert 'ngcf.hip' in open(os.path.join(PACKAGE, 'csrc', 'Makefile')).read()
    handle = lib.lib()
    assert handle.sbr_abi_version() == 4
    for e, n_args in zip(ENTRIES, (22, 29)):
        fn = getattr(handle, e)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args
    ws = handle.sbr_ngcf_layer_bwd_workspace
    assert ws.restype is ctypes.c_long
    assert ws(0, 64, 64) == 0 and ws(100, 129, 64) == 0 and ws(100, 64, 64) == 2 * 4 * (2 * 64 * 64 + 64)
