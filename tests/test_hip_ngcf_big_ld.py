"""Address arithmetic past 2^31 and 2^32 elements in NGCF's layer entries (csrc/ngcf.hip): `out` of 'sbr_ngcf_layer_fwd' and `g_out` of
'sbr_ngcf_layer_bwd' are column slices of the concatenated representation, addressed as row * out_ld, and a catalogue of 8.4 M joint
rows at 256 columns is past 2^31 elements. The scheme of tests/test_hip_big_ld.py: the slice is a view of 130 joint rows at LD_BIG =
2^25 + 64 inside the one untouched 16.1 GiB buffer, everything else is compact; the results equal the same calls on a compact slice bit
for bit, and the guard bands around the rows keep their bits."""
import numpy as np
import pytest
import torch

import lightgcn_ref as L
import ngcf_ref as R
from hip_testutil import BIG_ROWS, DEV, LD_BIG, S, _BigLd, _assert_bits, call, stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def big_buffer():
    """the one large allocation of the module (skips the module when the device has no room for it), freed at the end"""
    _BigLd._flat()
    yield
    _BigLd.release()


@pytest.mark.parametrize('width', [(5, 3), (64, 128)], ids=lambda w: f'{w[0]}x{w[1]}')
def test_the_slice_at_a_leading_dimension_past_2_to_31(width):
    from importlib import import_module
    din, dout = width
    g = L.world(65, BIG_ROWS - 65)
    assert g.n == BIG_ROWS
    ops = S().ops
    csr = import_module(ops.__name__.rsplit('.', 1)[0] + '.features').DeviceCSR(g.m).to(DEV)
    ti, tx, _ = csr.transposed()
    graph = [csr.indptr.data_ptr(), csr.indices.data_ptr(), ti.data_ptr(), tx.data_ptr(), g.n_users, g.n_items]
    W1n, W2n, bn = R.weights(din, dout)
    x, W1, W2, bias = (torch.from_numpy(t).to(DEV) for t in (L.table(g.n, din, 11), W1n, W2n, bn))
    h_ref, out_ref = ops.ngcf_layer(csr, x, W1, W2, bias, R.SLOPE, 0.3, R.SEED, R.STREAM)
    big = _BigLd(g.n, dout)
    assert all(big.crossings.values())
    h = torch.empty(g.n, dout, device=DEV)
    call('sbr_ngcf_layer_fwd', *graph, 0, g.n, x.data_ptr(), din, W1.data_ptr(), W2.data_ptr(), bias.data_ptr(), dout, R.SLOPE, 0.3, R.SEED, R.STREAM,
         h.data_ptr(), big.ptr, LD_BIG, stream())
    _assert_bits(big.check_untouched(what='out at LD_BIG'), out_ref.cpu(), 'out at LD_BIG')
    _assert_bits(h.cpu(), h_ref.cpu(), 'h beside out at LD_BIG')
    # backward: g_out read through the same view (its values are the forward's out)
    want = ops.ngcf_layer_bwd(csr, x, W1, W2, h_ref, out_ref, None, R.SLOPE, 0.3, R.SEED, R.STREAM)
    ds, dxd = torch.empty(g.n, din, device=DEV), torch.empty(g.n, din, device=DEV)
    dW1, dW2, db = torch.empty(din, dout, device=DEV), torch.empty(din, dout, device=DEV), torch.empty(dout, device=DEV)
    ws = torch.zeros(1 << 18, device=DEV)
    call('sbr_ngcf_layer_bwd', *graph, 0, g.n, x.data_ptr(), din, W1.data_ptr(), W2.data_ptr(), dout, R.SLOPE, 0.3, R.SEED, R.STREAM, h.data_ptr(),
         big.ptr, LD_BIG, None, ds.data_ptr(), dxd.data_ptr(), dW1.data_ptr(), dW2.data_ptr(), db.data_ptr(), ws.data_ptr(), 4 * ws.numel(), stream())
    _assert_bits(big.check_untouched(what='g_out at LD_BIG'), out_ref.cpu(), 'g_out is read, not written')
    for name, got, ref in zip(('ds', 'dx_direct', 'dW1', 'dW2', 'dbias'), (ds, dxd, dW1, dW2, db), want):
        _assert_bits(got.cpu(), ref.cpu(), name + ' with g_out at LD_BIG')
