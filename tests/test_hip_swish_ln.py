"""RecVAE's layer tail on the GPU: the entries 'sbr_swish_ln_fwd' and 'sbr_swish_ln_bwd' (csrc/recvae.hip; 'sbr_swish_ln_slabs' sizes the
backward pass's partials) through the C ABI on _Buf operands, against the float64 definitions inside the bound derived in
tests/recvae_ref.py: every width at which the elements-per-lane count or the tail of the last lane group changes, every batch size at the
tails of the rows-per-workgroup count and of the column slabs, the running sum present and NULL on either side, either gradient NULL,
the large-mean row and the exactly constant row; a row's bits under its position, B and the run; refusals; ``ops.SwishLayerNormFn``."""
import numpy as np
import pytest
import torch

import recvae_ref as R
from hip_testutil import DEV, S, _Buf, _assert_bits, _L, call, stream

pytestmark = pytest.mark.gpu
FWD, BWD, SLABS = 'sbr_swish_ln_fwd', 'sbr_swish_ln_bwd', 'sbr_swish_ln_slabs'
EPS = R.LN_EPS


def slabs(B):
    return int(_L().lib().sbr_swish_ln_slabs(B))


def buf(x, B, W):
    return None if x is None else _Buf(B, W, data=torch.from_numpy(np.ascontiguousarray(x)).reshape(B, W))


def forward(a, r, gamma, beta, want_sum=True):
    """the forward entry on _Buf operands -> dict of host tensors (r_out None when not asked for), after the guard checks"""
    B, H = a.shape
    ins = [buf(a, B, H), buf(r, B, H), buf(gamma, 1, H), buf(beta, 1, H)]
    s, h, ro, mean, rstd = _Buf(B, H), _Buf(B, H), (_Buf(B, H) if want_sum else None), _Buf(1, B), _Buf(1, B)
    call(FWD, ins[0].ptr, ins[1].ptr if r is not None else None, ins[2].ptr, ins[3].ptr, EPS, B, H, s.ptr, h.ptr, ro.ptr if want_sum else None,
         mean.ptr, rstd.ptr, stream())
    what = f'B = {B}, H = {H}'
    for b, x in zip(ins, (a, r, gamma, beta)):
        if b is not None:
            _assert_bits(b.check_untouched(what=what), torch.from_numpy(x).reshape(b.rows, b.cols), what + ': an input was written')
    return dict(s=s.check_untouched(what=what), h=h.check_untouched(what=what), r_out=ro.check_untouched(what=what) if want_sum else None,
                mean=mean.check_untouched(what=what)[0], rstd=rstd.check_untouched(what=what)[0])


def backward(f, gamma, dh, dr, want_dr_in=True, colsums=True):
    B, H = f['s'].shape
    ins = [buf(f['s'].numpy(), B, H), buf(f['mean'].numpy(), 1, B), buf(f['rstd'].numpy(), 1, B), buf(gamma, 1, H), buf(dh, B, H), buf(dr, B, H)]
    da, dri = _Buf(B, H), (_Buf(B, H) if want_dr_in else None)
    dg, db, part = (_Buf(1, H), _Buf(1, H), _Buf(1, slabs(B) * 2 * H)) if colsums else (None, None, None)
    call(BWD, ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, ins[4].ptr if dh is not None else None, ins[5].ptr if dr is not None else None, B, H,
         da.ptr, dri.ptr if want_dr_in else None, dg.ptr if colsums else None, db.ptr if colsums else None, part.ptr if colsums else None, stream())
    what = f'B = {B}, H = {H} backward'
    out = dict(da=da.check_untouched(what=what), dr_in=dri.check_untouched(what=what) if want_dr_in else None)
    if colsums:
        part.check_untouched(what=what)
        out.update(dgamma=dg.check_untouched(what=what)[0], dbeta=db.check_untouched(what=what)[0])
    return out


def variants(r, dh, dr):
    """(r_in, want r_out, dh, dr_out)"""
    return [(r, True, dh, dr), (None, True, dh, dr), (r, False, dh, None), (r, True, None, dr), (None, False, dh, None)]


# ---- 1. against float64, inside the bound ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', R.BATCHES)
@pytest.mark.parametrize('H', R.H_SIZES)
def test_against_float64_inside_the_bound(H, B):
    ops = S().ops
    a, r, gamma, beta, dh, dr = R.swish_ln_case(B, H, 0)
    before = ops.nondeterministic_launches()
    worst = {}
    for r_in, want_sum, g_h, g_r in variants(r, dh, dr):
        bound = R.swish_ln_bound(a, r_in, gamma, beta, EPS, g_h, g_r)
        f = forward(a, r_in, gamma, beta, want_sum)
        g = backward(f, gamma, g_h, g_r, want_dr_in=r_in is not None)
        got = {**f, **g}
        for k, v in got.items():
            if v is not None:
                worst[k] = max(worst.get(k, 0.0), R.ratio(v.double().numpy(), bound[k]))
        for b in range(B):
            # the exactly constant row: h = beta and rstd = 1 / sqrt(eps), inside the bound at every width (checked above: float64 has
            # a variance of exactly 0 there) and bit for bit where the row's sum is exact (one element per lane: only doublings)
            if b % 5 == 2 and H in (1, 2, 64):
                _assert_bits(f['h'][b], torch.from_numpy(beta), 'a constant row gives beta')
                assert float(f['rstd'][b]) == float(np.float32(1) / np.sqrt(np.float32(EPS)))
        f2 = forward(a, r_in, gamma, beta, want_sum)
        g2 = backward(f2, gamma, g_h, g_r, want_dr_in=r_in is not None)
        for k, v in {**f2, **g2}.items():
            if v is not None:
                _assert_bits(v, got[k], f'second run: {k}')
        g3 = backward(f, gamma, g_h, g_r, want_dr_in=False, colsums=False)
        _assert_bits(g3['da'], g['da'], 'without column sums and dr_in: da')
    print(f'H = {H}, B = {B}: largest error / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    assert ops.nondeterministic_launches() == before, 'an entry counted as a nondeterministic launch'


# ---- 2. a row's bits do not depend on where it stands -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', [1, 65, 600, 1024])
def test_a_row_has_the_same_bits_everywhere(H):
    ops = S().ops
    a1, r1, gamma, beta, dh1, dr1 = R.swish_ln_case(1, H, 7)
    f_ref = forward(a1, r1, gamma, beta)
    g_ref = backward(f_ref, gamma, dh1, dr1, colsums=False)
    for B, at in ((3, 2), (4, 3), (5, 4), (67, 0), (67, 65)):
        a, r, _, _, dh, dr = R.swish_ln_case(B, H, B)
        a[at], r[at], dh[at], dr[at] = a1[0], r1[0], dh1[0], dr1[0]
        f = forward(a, r, gamma, beta)
        g = backward(f, gamma, dh, dr)
        for k in ('s', 'h', 'r_out', 'mean', 'rstd'):
            _assert_bits(f[k][at:at + 1], f_ref[k], f'B = {B}, position {at}: {k}')
        for k in ('da', 'dr_in'):
            _assert_bits(g[k][at:at + 1], g_ref[k], f'B = {B}, position {at}: {k}')
    prev = ops.set_deterministic(True)
    try:
        f_det = forward(a1, r1, gamma, beta)
        g_det = backward(f_det, gamma, dh1, dr1)
    finally:
        ops.set_deterministic(prev)
    for k in ('s', 'h', 'r_out', 'mean', 'rstd'):
        _assert_bits(f_det[k], f_ref[k], 'deterministic mode on: ' + k)
    _assert_bits(g_det['da'], g_ref['da'], 'deterministic mode on: da')


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    Sm = S()
    B, H = 4, 68
    a, r, gamma, beta, dh, dr = R.swish_ln_case(B, H, 1)
    bufs = dict(a=buf(a, B, H), r=buf(r, B, H), gamma=buf(gamma, 1, H), beta=buf(beta, 1, H), s=_Buf(B, H, fill=1.5), h=_Buf(B, H, fill=2.5),
                ro=_Buf(B, H, fill=3.5), mean=_Buf(1, B, fill=4.5), rstd=_Buf(1, B, fill=5.5), dh=buf(dh, B, H), dr=buf(dr, B, H),
                da=_Buf(B, H, fill=6.5), dri=_Buf(B, H, fill=7.5), dg=_Buf(1, H, fill=8.5), db=_Buf(1, H, fill=9.5),
                part=_Buf(1, slabs(B) * 2 * H, fill=10.5))
    before = {k: b.flat.clone() for k, b in bufs.items()}
    p = {k: b.ptr for k, b in bufs.items()}

    def untouched(why):
        for k, b in bufs.items():
            assert torch.equal(b.flat.view(torch.int32), before[k].view(torch.int32)), f'{why}: {k} was written'

    def fwd(B=B, H=H, eps=EPS, **change):
        q = {**p, **change}
        call(FWD, q['a'], q['r'], q['gamma'], q['beta'], eps, B, H, q['s'], q['h'], q['ro'], q['mean'], q['rstd'], stream())

    def bwd(B=B, H=H, **change):
        q = {**p, **change}
        call(BWD, q['s'], q['mean'], q['rstd'], q['gamma'], q['dh'], q['dr'], B, H, q['da'], q['dri'], q['dg'], q['db'], q['part'], stream())

    for entry, fn, cases in ((FWD, fwd, [dict(a=None), dict(gamma=None), dict(beta=None), dict(s=None), dict(h=None), dict(mean=None),
                                         dict(rstd=None), dict(H=0), dict(H=1025), dict(H=-1), dict(B=-1), dict(eps=0.0), dict(eps=float('nan'))]),
                             (BWD, bwd, [dict(s=None), dict(mean=None), dict(rstd=None), dict(gamma=None), dict(da=None), dict(dh=None, dr=None),
                                         dict(dg=None), dict(db=None), dict(part=None), dict(dg=None, db=None), dict(H=0), dict(H=1025),
                                         dict(B=-1)])):
        for change in cases:
            with pytest.raises(Sm.SibrarHipError, match=entry):
                fn(**change)
            untouched(f'{entry} {change}')
    fwd(B=0)
    bwd(B=0)
    untouched('B = 0')
    assert slabs(0) == 0 and slabs(-3) == 0 and slabs(1) == 1 and slabs(4) == 1 and slabs(5) == 2 and slabs(67) == 17 == R.slabs(67)
    assert slabs(4096) == 1024 and slabs(4097) == 513 == R.slabs(4097)


# ---- 4. the autograd function --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_sum', [True, False])
def test_autograd_function(with_sum):
    ops = S().ops
    B, H = 5, 65
    a, r, gamma, beta, dh, dr = R.swish_ln_case(B, H, 3, with_sum)
    t = {k: torch.from_numpy(v).to(DEV).requires_grad_() for k, v in dict(a=a, gamma=gamma, beta=beta).items()}
    rt = torch.from_numpy(r).to(DEV).requires_grad_() if with_sum else None
    h, ro = ops.SwishLayerNormFn.apply(t['a'], rt, t['gamma'], t['beta'], EPS, True)
    ((h * torch.from_numpy(dh).to(DEV)).sum() + (ro * torch.from_numpy(dr).to(DEV)).sum()).backward()
    bound = R.swish_ln_bound(a, r, gamma, beta, EPS, dh, dr)
    got = dict(h=h, r_out=ro, da=t['a'].grad, dgamma=t['gamma'].grad, dbeta=t['beta'].grad)
    if with_sum:
        got['dr_in'] = rt.grad
    q = {k: R.ratio(v.detach().cpu().double().numpy(), bound[k]) for k, v in got.items()}
    assert max(q.values()) <= 1.0, q
    # only h is used, no running sum is asked for: dr_out never exists
    t2 = torch.from_numpy(a).to(DEV).requires_grad_()
    h2, none = ops.SwishLayerNormFn.apply(t2, rt, t['gamma'], t['beta'], EPS, False)
    assert none is None
    _assert_bits(h2.detach().cpu(), h.detach().cpu(), 'want_sum = False: h')
    (h2 * torch.from_numpy(dh).to(DEV)).sum().backward()
    only_h = R.swish_ln_bound(a, r, gamma, beta, EPS, dh, None)
    assert R.ratio(t2.grad.cpu().double().numpy(), only_h['da']) <= 1.0
    with pytest.raises(ValueError, match='contiguous float32'):
        ops.SwishLayerNormFn.apply(t['a'], rt, t['gamma'][:H - 1], t['beta'], EPS, True)
    with pytest.raises(S().SibrarHipError, match=FWD):
        ops.SwishLayerNormFn.apply(torch.zeros(2, 1025, device=DEV), None, torch.ones(1025, device=DEV), torch.zeros(1025, device=DEV), EPS, True)
