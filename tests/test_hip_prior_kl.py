"""RecVAE's composite-prior KL on the GPU: the entries 'sbr_prior_kl_fwd' and 'sbr_prior_kl_bwd' (csrc/recvae.hip) through the C ABI on
_Buf operands, against the float64 definitions inside the bound derived in tests/recvae_ref.py: every width at which the
elements-per-lane count or the last lane group's tail changes, the batch sizes at the tails of the rows-per-workgroup count, weights with
zeros, logvar_old in {-20, 0, 10}, |z| up to 50; z bit for bit the restatement's float32 ``mu + eps * E(0.5 logvar)``; a row's bits under
its position, B and the run; refusals; ``ops.CompositePriorKLFn``."""
import numpy as np
import pytest
import torch

import recvae_ref as R
from hip_testutil import DEV, S, _Buf, _assert_bits, call, stream

pytestmark = pytest.mark.gpu
FWD, BWD = 'sbr_prior_kl_fwd', 'sbr_prior_kl_bwd'
NAMES = ('mu', 'logvar', 'eps', 'mu_old', 'logvar_old')


def buf(x, rows, cols):
    return None if x is None else _Buf(rows, cols, data=torch.from_numpy(np.ascontiguousarray(x)).reshape(rows, cols))


def run(case, dz=None, upstream=None, scale=0.0, backward=True):
    """both entries on _Buf operands -> dict(z, row_kl, dmu, dlogvar) of host tensors, after the guard and input checks"""
    mu, logvar, eps, mu_old, logvar_old, weight = case
    B, L = mu.shape
    ins = {n: buf(x, B, L) for n, x in zip(NAMES, case)}
    ins['weight'] = buf(weight, 1, B)
    z, row = _Buf(B, L), _Buf(1, B)
    call(FWD, *(ins[n].ptr for n in NAMES), ins['weight'].ptr, B, L, z.ptr, row.ptr, stream())
    what = f'B = {B}, L = {L}'
    out = dict(z=z.check_untouched(what=what), row_kl=row.check_untouched(what=what)[0])
    if backward:
        zin, dzb = buf(out['z'].numpy(), B, L), buf(dz, B, L)
        up = None if upstream is None else torch.tensor([upstream], dtype=torch.float32, device=DEV)
        dmu, dlv = _Buf(B, L), _Buf(B, L)
        call(BWD, *(ins[n].ptr for n in NAMES[1:]), ins['weight'].ptr, zin.ptr, dzb.ptr if dz is not None else None,
             up.data_ptr() if up is not None else None, float(scale), B, L, dmu.ptr, dlv.ptr, stream())
        out.update(dmu=dmu.check_untouched(what=what), dlogvar=dlv.check_untouched(what=what))
        _assert_bits(zin.check_untouched(what=what), out['z'], what + ': z was written by the backward pass')
    for n, x in zip(NAMES + ('weight',), case):
        _assert_bits(ins[n].check_untouched(what=what), torch.from_numpy(x).reshape(ins[n].rows, ins[n].cols), what + f': {n} was written')
    return out


# ---- 1. against float64, inside the bound ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', R.BATCHES)
@pytest.mark.parametrize('L', R.L_SIZES)
def test_against_float64_inside_the_bound(L, B):
    ops = S().ops
    *case, dz = R.prior_kl_case(B, L, 0)
    assert set(np.unique(case[4])) <= {-20.0, 0.0, 10.0} and (B == 1 or (case[5] == 0).any())
    before = ops.nondeterministic_launches()
    worst = {}
    for g_z, up, scale in ((dz, 0.7, 1.0 / B), (None, None, 1.0 / B), (dz, None, 0.0)):
        bound = R.prior_kl_bound(*case, g_z, up, scale)
        got = run(case, g_z, up, scale)
        for k, v in got.items():
            worst[k] = max(worst.get(k, 0.0), R.ratio(v.double().numpy(), bound[k]))
        _assert_bits(got['z'], torch.from_numpy(R.z32(*case[:3])), 'z against the float32 restatement')
        again = run(case, g_z, up, scale)
        for k, v in again.items():
            _assert_bits(v, got[k], f'second run: {k}')
    zmax = float(np.abs(R.z32(*case[:3])).max())
    print(f'L = {L}, B = {B}: |z| up to {zmax:.1f}; largest error / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    assert zmax < 50.5
    assert ops.nondeterministic_launches() == before, 'an entry counted as a nondeterministic launch'


def test_the_extremes_stay_finite():
    z = np.array([[-50.0, 50.0, 0.0, 1e-5, 49.0, -3.0]], dtype=np.float32)
    zero = np.zeros_like(z)
    for lvo in (-20.0, 0.0, 10.0):
        for mo in (0.0, 50.0):
            case = (z, zero, zero, zero + np.float32(mo), zero + np.float32(lvo), np.ones(1, dtype=np.float32))
            got = run(case, None, 1.0, 1.0)
            assert all(bool(torch.isfinite(v).all()) for v in got.values()), (lvo, mo)
            bound = R.prior_kl_bound(*case, None, 1.0, 1.0)
            q = {k: R.ratio(v.double().numpy(), bound[k]) for k, v in got.items()}
            assert max(q.values()) <= 1.0, (lvo, mo, q)


# ---- 2. a row's bits do not depend on where it stands -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', [1, 65, 200, 1024])
def test_a_row_has_the_same_bits_everywhere(L):
    ops = S().ops
    *one, dz1 = R.prior_kl_case(1, L, 7)
    one[5][:] = 0.625
    ref = run(one, dz1, 0.5, 0.25)
    for B, at in ((3, 2), (4, 3), (5, 4), (67, 0), (67, 65)):
        *case, dz = R.prior_kl_case(B, L, B)
        for k in range(6):
            case[k][at] = one[k][0]
        dz[at] = dz1[0]
        got = run(case, dz, 0.5, 0.25)                                     # the same upstream * scale: the row's gradients are the same too
        for k in ('z', 'dmu', 'dlogvar'):
            _assert_bits(got[k][at:at + 1], ref[k], f'B = {B}, position {at}: {k}')
        _assert_bits(got['row_kl'][at:at + 1], ref['row_kl'], f'B = {B}, position {at}: row_kl')
    prev = ops.set_deterministic(True)
    try:
        det = run(one, dz1, 0.5, 0.25)
    finally:
        ops.set_deterministic(prev)
    for k, v in det.items():
        _assert_bits(v, ref[k], 'deterministic mode on: ' + k)


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    Sm = S()
    B, L = 4, 68
    *case, dz = R.prior_kl_case(B, L, 1)
    bufs = {n: buf(x, B, L) for n, x in zip(NAMES, case)}
    bufs.update(weight=buf(case[5], 1, B), z=_Buf(B, L, fill=1.5), row=_Buf(1, B, fill=2.5), dz=buf(dz, B, L), dmu=_Buf(B, L, fill=3.5),
                dlv=_Buf(B, L, fill=4.5))
    before = {k: b.flat.clone() for k, b in bufs.items()}
    p = {k: b.ptr for k, b in bufs.items()}

    def untouched(why):
        for k, b in bufs.items():
            assert torch.equal(b.flat.view(torch.int32), before[k].view(torch.int32)), f'{why}: {k} was written'

    def fwd(B=B, L=L, **change):
        q = {**p, **change}
        call(FWD, *(q[n] for n in NAMES), q['weight'], B, L, q['z'], q['row'], stream())

    def bwd(B=B, L=L, **change):
        q = {**p, **change}
        call(BWD, *(q[n] for n in NAMES[1:]), q['weight'], q['z'], q['dz'], None, 0.25, B, L, q['dmu'], q['dlv'], stream())

    sizes = [dict(L=0), dict(L=1025), dict(L=-1), dict(B=-1)]
    for entry, fn, cases in ((FWD, fwd, [{n: None} for n in NAMES + ('weight', 'z', 'row')] + sizes),
                             (BWD, bwd, [{n: None} for n in NAMES[1:] + ('weight', 'z', 'dmu', 'dlv')] + sizes)):
        for change in cases:
            with pytest.raises(Sm.SibrarHipError, match=entry):
                fn(**change)
            untouched(f'{entry} {change}')
    fwd(B=0)
    bwd(B=0)
    untouched('B = 0')


# ---- 4. the autograd function --------------------------------------------------------------------------------------------------------------------
def test_autograd_function():
    ops = S().ops
    B, L = 5, 65
    *case, dz = R.prior_kl_case(B, L, 3)
    t = [torch.from_numpy(x).to(DEV) for x in case]
    mu, logvar = t[0].requires_grad_(), t[1].requires_grad_()
    z, kl = ops.CompositePriorKLFn.apply(mu, logvar, *t[2:])
    ((z * torch.from_numpy(dz).to(DEV)).sum() + 0.7 * kl).backward()
    bound = R.prior_kl_bound(*case, dz, 0.7, 1.0 / B)
    q = {k: R.ratio(v.detach().cpu().double().numpy(), bound[k]) for k, v in dict(z=z, dmu=mu.grad, dlogvar=logvar.grad).items()}
    assert max(q.values()) <= 1.0, q
    # the scalar: the mean of row_kl; any summation order of B terms stays inside gamma(B) of their magnitudes, and one division
    row = bound['row_kl']
    err = row.e.sum() + R.gamma_k(B) * (np.abs(row.v).sum() + row.e.sum())
    err = (err + R.U * (abs(row.v.sum()) + err)) / B
    assert abs(float(kl.detach()) - row.v.mean()) <= err, (float(kl.detach()), row.v.mean(), err)
    assert all(x.grad is None for x in t[2:])
    # kl alone, z unused; z alone, kl unused
    for use_z, use_kl in ((False, True), (True, False)):
        m2, l2 = t[0].detach().clone().requires_grad_(), t[1].detach().clone().requires_grad_()
        z2, kl2 = ops.CompositePriorKLFn.apply(m2, l2, *t[2:])
        ((z2 * torch.from_numpy(dz).to(DEV)).sum() if use_z else kl2 * 1.0).backward()
        b2 = R.prior_kl_bound(*case, dz if use_z else None, 1.0 if use_kl else None, 1.0 / B if use_kl else 0.0)
        assert R.ratio(m2.grad.cpu().double().numpy(), b2['dmu']) <= 1.0 and R.ratio(l2.grad.cpu().double().numpy(), b2['dlogvar']) <= 1.0
    with pytest.raises(ValueError, match='contiguous float32'):
        ops.CompositePriorKLFn.apply(mu, logvar[:, :L - 1], *t[2:])
    with pytest.raises(ValueError, match='weight'):
        ops.CompositePriorKLFn.apply(mu, logvar, t[2], t[3], t[4], t[5][:B - 1])
