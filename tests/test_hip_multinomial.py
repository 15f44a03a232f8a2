"""The multinomial likelihood kernel on the GPU: the entry 'sbr_multinomial_nll_f32' (csrc/multinomial.hip) through the C ABI on
_Buf operands against float64 inside the bound derived in tests/multvae_ref.py, at every dispatch boundary (a wave per row up to 1,024
items, a workgroup with the row in LDS up to 12,288, a workgroup that reads the row twice above), aligned and one float off the 16-byte
boundary, in place and out of place; exact cases; invariance of a row's bits under its position, its neighbours, B and the run; one case
past 2^31 elements; refusals."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import multvae_ref as R
from hip_testutil import DEV, S, _Buf, _assert_bits, _i32, _i64, call, stream

pytestmark = pytest.mark.gpu
ENTRY = 'sbr_multinomial_nll_f32'
N_ITEMS = [1, 3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1027, 1028, 4100, 12287, 12288, 12289, 12292]
BATCHES = [1, 2, 5, 257]
KINDS = ('normal', 'wide', 'constant', 'spike')


def users(n_items, seed=0):
    """a users x items 0/1 matrix whose rows have the degrees 0, 1, a few, n_items and some in between -> (csr, dense float64)"""
    rng = np.random.default_rng(seed)
    degs = sorted({0, 1, min(3, n_items), min(17, n_items), n_items // 2, n_items, min(300, n_items)})
    dense = np.zeros((len(degs), n_items))
    for r, d in enumerate(degs):
        dense[r, rng.choice(n_items, size=d, replace=False)] = 1
    m = sp.csr_matrix(dense)
    m.sort_indices()
    return m, dense


def logits_of(kind, B, n_items, seed):
    rng = np.random.default_rng(seed)
    if kind == 'normal':
        z = rng.standard_normal((B, n_items))
    elif kind == 'wide':
        z = 30 * rng.standard_normal((B, n_items))                     # most exponentials underflow
    elif kind == 'constant':
        z = np.repeat(rng.standard_normal((B, 1)), n_items, axis=1)
    else:
        z = np.full((B, n_items), -80.0)
        z[np.arange(B), rng.integers(0, n_items, size=B)] = 80.0
    return z.astype(np.float32)


class Csr:
    def __init__(self, m):
        self.indptr, self.indices = _i64(m.indptr), _i32(m.indices)


def run(csr, rows, z, gs, off=0, inplace=False, forward_only=False, lse=True):
    """the entry on _Buf operands -> (row_loss, row_lse or None, dlogits or None) on the host, after the guard and input checks"""
    B, I = z.shape
    zt = torch.from_numpy(z)
    lg, loss, ls = _Buf(B, I, off=off, data=zt), _Buf(1, B, off=off), _Buf(1, B, off=off)
    dl = None if (inplace or forward_only) else _Buf(B, I, off=off)
    dptr = None if forward_only else (lg.ptr if inplace else dl.ptr)
    call(ENTRY, csr.indptr.data_ptr(), csr.indices.data_ptr(), rows.data_ptr(), B, I, lg.ptr, dptr, float(gs), loss.ptr,
         ls.ptr if lse else None, stream())
    what = f'B = {B}, n_items = {I}, off = {off}, inplace = {inplace}'
    got_loss = loss.check_untouched(what=what + ': row_loss')[0]
    got_lse = ls.check_untouched(what=what + ': row_lse')[0]
    if not lse:
        assert bool(torch.isnan(got_lse).all()), 'row_lse = NULL was written'
    got_z = lg.check_untouched(what=what + ': logits')
    if inplace:
        return got_loss, got_lse if lse else None, got_z
    _assert_bits(got_z, zt, what + ': logits were written')
    return got_loss, got_lse if lse else None, None if forward_only else dl.check_untouched(what=what + ': dlogits')


def ratio(got, ref, bound):
    err = np.abs(got.double().numpy() - ref)
    assert np.isfinite(err).all()
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(q.max()) if q.size else 0.0


# ---- 1. every dispatch branch against float64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('n_items', N_ITEMS)
def test_against_float64_inside_the_bound(n_items, B):
    m, dense = users(n_items)
    csr = Csr(m)
    rng = np.random.default_rng(B)
    order = [m.shape[0] - 1, 0] + list(range(1, m.shape[0] - 1))         # the full row and the empty row first: every B has them (B = 1: the full row)
    rows_h = rng.permutation(np.resize(order, B))
    rows = _i64(rows_h)
    t = dense[rows_h]
    gs = np.float32(1.0 / B)
    worst = {}
    for k, kind in enumerate(KINDS):
        z = logits_of(kind, B, n_items, 10 * B + k)
        loss64, lse64, d64 = R.nll64(z, t, gs)
        eloss, else_, ed = R.nll_bound(z, t, gs)
        loss, lse, d = run(csr, rows, z, gs)
        q = (ratio(loss, loss64, eloss), ratio(lse, lse64, else_), ratio(d, d64, ed))
        rowsum = np.abs(d.double().numpy().sum(1))
        q += (float((rowsum / np.maximum(ed.sum(1), 1e-300)).max()),)
        worst[kind] = q
        assert max(q) <= 1.0, f'{kind}: error / bound of (row_loss, row_lse, dlogits, row sums of dlogits) = {q}'
        empty = t.sum(1) == 0
        assert not bool(loss.view(torch.int32)[torch.from_numpy(empty)].any()) and not bool(d.view(torch.int32)[torch.from_numpy(empty)].any()), \
            'a row without items must give +0.0f everywhere'
        # one float off the 16-byte boundary: the four-float chunks, the same bits; in place: the same bits
        for off, inplace in ((1, False), (0, True), (1, True)):
            l2, s2, d2 = run(csr, rows, z, gs, off=off, inplace=inplace)
            what = f'{kind}, off = {off}, inplace = {inplace}'
            _assert_bits(l2, loss, what + ': row_loss')
            _assert_bits(s2, lse, what + ': row_lse')
            _assert_bits(d2, d, what + ': dlogits')
    print(f'n_items = {n_items}, B = {B}: largest error / bound (row_loss, row_lse, dlogits, row sums) ' +
          ', '.join(f'{k}: ' + '/'.join(f'{v:.3f}' for v in q) for k, q in worst.items()))


# ---- 2. exact cases and the optional operands ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_items', [1, 65, 1028, 4100, 12289])
def test_zero_scale_forward_only_and_no_lse(n_items):
    m, dense = users(n_items)
    csr = Csr(m)
    rows = _i64(np.arange(m.shape[0]))
    z = logits_of('normal', m.shape[0], n_items, 5)
    loss, lse, d = run(csr, rows, z, 0.5)
    l0, s0, d0 = run(csr, rows, z, 0.0)
    assert not bool(d0.view(torch.int32).any()), 'grad_scale = 0 must give +0.0f everywhere'
    _assert_bits(l0, loss, 'row_loss does not depend on grad_scale')
    lf, sf, df = run(csr, rows, z, 0.5, forward_only=True)
    assert df is None
    _assert_bits(lf, loss, 'forward only: row_loss')
    _assert_bits(sf, lse, 'forward only: row_lse')
    ln, sn, dn = run(csr, rows, z, 0.5, lse=False)
    assert sn is None
    _assert_bits(ln, loss, 'row_lse = NULL: row_loss')
    _assert_bits(dn, d, 'row_lse = NULL: dlogits')
    if n_items == 1:                                                     # lse = z exactly, loss and gradient exactly zero
        _assert_bits(lse, torch.from_numpy(z[:, 0]), 'n_items = 1: lse is the logit')
        assert not bool(loss.any()) and not bool(d.any())


# ---- 3. a row's bits do not depend on where it stands --------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_items', [65, 1024, 1027, 4100, 12292])
def test_a_row_has_the_same_bits_everywhere(n_items):
    ops = S().ops
    m, _ = users(n_items)
    csr = Csr(m)
    row = logits_of('normal', 1, n_items, 77)
    user = m.shape[0] - 3
    before = ops.nondeterministic_launches()
    ref = run(csr, _i64([user]), row, 0.25)
    for B, at, seed in ((5, 3, 1), (257, 200, 2), (257, 0, 3), (2, 1, 4)):
        z = logits_of('wide' if seed % 2 else 'normal', B, n_items, seed)
        z[at] = row[0]
        rows_h = np.random.default_rng(seed).integers(0, m.shape[0], size=B)
        rows_h[at] = user
        for inplace in (False, True):
            loss, lse, d = run(csr, _i64(rows_h), z, 0.25, inplace=inplace)
            what = f'B = {B}, position {at}, inplace = {inplace}'
            _assert_bits(loss[at:at + 1], ref[0], what + ': row_loss')
            _assert_bits(lse[at:at + 1], ref[1], what + ': row_lse')
            _assert_bits(d[at:at + 1], ref[2], what + ': dlogits')
    prev = ops.set_deterministic(True)
    try:
        again = run(csr, _i64([user]), row, 0.25)
    finally:
        ops.set_deterministic(prev)
    for a, b, name in zip(again, ref, ('row_loss', 'row_lse', 'dlogits')):
        _assert_bits(a, b, 'second run, deterministic mode on: ' + name)
    assert ops.nondeterministic_launches() == before, 'the entry counted as a nondeterministic launch'


# ---- 4. past 2^31 elements -----------------------------------------------------------------------------------------------------------------------
def test_row_offsets_past_2_to_31_elements():
    I, B = (1 << 20) + 4, 2050
    assert (B - 1) * I > 1 << 31
    dense = np.zeros((3, I))
    rng = np.random.default_rng(9)
    for r, d in enumerate((0, 7, 1000)):
        dense[r, rng.choice(I, size=d, replace=False)] = 1
    m = sp.csr_matrix(dense)
    m.sort_indices()
    csr = Csr(m)
    rows_h = np.arange(B) % 3
    rows_h[[0, B // 2, B - 1]] = (2, 1, 2)
    rows, gs = _i64(rows_h), np.float32(1.0 / B)
    g = torch.Generator(device=DEV).manual_seed(4)
    z = torch.empty(B, I, device=DEV)
    zmax, zmin, lse64 = (torch.empty(B, dtype=torch.float64, device=DEV) for _ in range(3))
    for lo in range(0, B, 128):
        part = z[lo:lo + 128].normal_(generator=g)
        zmax[lo:lo + 128], zmin[lo:lo + 128] = part.max(1).values.double(), part.min(1).values.double()
        lse64[lo:lo + 128] = torch.logsumexp(part.double(), 1)
    probes = [0, B // 2, B - 1]
    kept = {b: z[b].cpu().numpy() for b in probes}
    loss, lse = torch.full((B,), float('nan'), device=DEV), torch.full((B,), float('nan'), device=DEV)
    call(ENTRY, csr.indptr.data_ptr(), csr.indices.data_ptr(), rows.data_ptr(), B, I, z.data_ptr(), z.data_ptr(), float(gs), loss.data_ptr(),
         lse.data_ptr(), stream())
    for b in probes:
        t = dense[rows_h[b]][None]
        loss64, l64, d64 = R.nll64(kept[b][None], t, gs)
        eloss, else_, ed = R.nll_bound(kept[b][None], t, gs)
        q = (ratio(loss[b:b + 1].cpu(), loss64, eloss), ratio(lse[b:b + 1].cpu(), l64, else_), ratio(z[b:b + 1].cpu(), d64, ed))
        print(f'row {b}: error / bound (row_loss, row_lse, dlogits) = {q}')
        assert max(q) <= 1.0, f'row {b}: {q}'
    sums = torch.cat([z[lo:lo + 128].double().sum(1) for lo in range(0, B, 128)]).abs().cpu().numpy()
    n = dense.sum(1)[rows_h]
    bound = R.coarse_row_sum_bound(I, n, zmax.cpu().numpy(), zmin.cpu().numpy(), lse64.cpu().numpy(), gs)
    assert (sums <= bound).all(), f'rows {np.nonzero(sums > bound)[0][:8]}: gradient row sums over the bound'
    assert not sums[n == 0].any() and not bool(loss[torch.from_numpy(n == 0).to(DEV)].any())
    assert ratio(lse.cpu(), lse64.cpu().numpy(), bound * 0 + 1e-3) <= 1.0 and not bool(torch.isnan(loss).any())


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    Sm = S()
    B, I = 4, 68
    m, _ = users(I)
    csr = Csr(m)
    rows = _i64(np.arange(B))
    lg, dl = _Buf(B, I, data=torch.from_numpy(logits_of('normal', B, I, 1))), _Buf(B, I, fill=7.25)
    loss, lse = _Buf(1, B, fill=-3.5), _Buf(1, B, fill=-4.5)
    before = [b.flat.clone() for b in (lg, dl, loss, lse)]
    ok = dict(indptr=csr.indptr.data_ptr(), indices=csr.indices.data_ptr(), rows=rows.data_ptr(), B=B, n_items=I, logits=lg.ptr, dlogits=dl.ptr,
              gs=0.5, row_loss=loss.ptr, row_lse=lse.ptr)

    def refused(**change):
        a = {**ok, **change}
        with pytest.raises(Sm.SibrarHipError, match=ENTRY):
            call(ENTRY, a['indptr'], a['indices'], a['rows'], a['B'], a['n_items'], a['logits'], a['dlogits'], a['gs'], a['row_loss'],
                 a['row_lse'], stream())
        for b, was in zip((lg, dl, loss, lse), before):
            assert torch.equal(b.flat.view(torch.int32), was.view(torch.int32)), f'{change}: an operand was written'

    for name in ('indptr', 'rows', 'logits', 'row_loss'):
        refused(**{name: None})
    refused(n_items=0)
    refused(n_items=-3)
    refused(B=-1)
    refused(dlogits=lg.ptr + 16)                                         # overlapping in part
    refused(dlogits=lg.ptr - 4 * I)
    refused(row_loss=lg.ptr + 8)
    refused(row_loss=dl.ptr + 4 * (B * I - 1))
    refused(row_lse=lg.ptr)
    refused(row_lse=dl.ptr + 64)
    refused(row_lse=loss.ptr + 4)
    # B == 0 returns at once
    call(ENTRY, ok['indptr'], ok['indices'], ok['rows'], 0, I, lg.ptr, dl.ptr, 0.5, loss.ptr, lse.ptr, stream())
    for b, was in zip((lg, dl, loss, lse), before):
        assert torch.equal(b.flat.view(torch.int32), was.view(torch.int32)), 'B = 0 wrote an operand'
    # the wrapper: a row id outside the matrix, a matrix with values, a strided logit matrix
    ops = Sm.ops
    features = __import__('importlib').import_module(ops.__name__.rsplit('.', 1)[0] + '.features')
    dcsr = features.DeviceCSR(m).to(DEV)
    z = torch.zeros(2, I, device=DEV)
    with pytest.raises(ValueError, match='row ids'):
        ops.multinomial_nll(dcsr, _i64([0, m.shape[0]]), z)
    with pytest.raises(ValueError, match='row ids'):
        ops.multinomial_nll(dcsr, _i64([-1, 0]), z)
    with pytest.raises(ValueError, match='0/1'):
        ops.multinomial_nll(features.DeviceCSR(m * 2.0).to(DEV), _i64([0, 1]), z)
    with pytest.raises(ValueError, match='contiguous'):
        ops.multinomial_nll(dcsr, _i64([0, 1]), torch.zeros(2, 2 * I, device=DEV)[:, :I])
    row_loss, row_lse = ops.multinomial_nll(dcsr, _i64([0, 1]), z)
    assert row_loss.shape == (2,) and row_lse.shape == (2,)
