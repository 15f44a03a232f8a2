"""'sbr_ultragcn_loss_fwd_bwd' (with 'sbr_ultragcn_loss_workspace') and 'sbr_scatter_add_scaled_rows_sorted' (csrc/ultragcn.hip,
``ops.UltraGCNLossFn``) on the GPU against float64 under the derived bound of tests/ultragcn_ref.py (c): the three parts, the total, the
scores, dUb, the coefficient matrix and the item-table gradient, on batches that repeat users and items, name an item as positive,
negative and neighbour at once, hold lists shorter than K and reach scores near +-30. Bit equality of two runs and of the item-table
gradient with the numpy float32 order oracle; the refusals; a NaN guard row that a padded -1 slot would reach as a wrapped index.

Largest error / bound ratios measured on an MI355X (printed by the test): see DESIGN.md §4.34."""
import numpy as np
import pytest
import torch

import ultragcn_ref as R
from hip_testutil import DEV, S, _Buf, _assert_bits, call, stream

pytestmark = pytest.mark.gpu
# (D, B, N, K): every D, B, N and K of the issue at least once; both chunk widths, one and several rows per wave, a partial last wave
CASES = [(1, 1, 1, 1), (3, 2, 7, 10), (64, 65, 300, 10), (100, 257, 7, 64), (256, 2, 300, 64), (64, 257, 1, 1)]
ORACLE_MAX_SLOTS = 6000                      # the order oracle is a Python loop over the slots


def guarded(c):
    """the case with one more item row that nothing names: NaN in the table, its beta and its list. A -1 used as an index would wrap to it."""
    g = dict(c)
    K = c['nbr_idx'].shape[1]
    g['V'] = np.concatenate([c['V'], np.full((1, c['V'].shape[1]), np.nan, dtype=np.float32)])
    g['beta_i'] = np.concatenate([c['beta_i'], np.array([np.nan], dtype=np.float32)])
    g['nbr_idx'] = np.concatenate([c['nbr_idx'], np.full((1, K), c['V'].shape[0], dtype=np.int32)])
    g['nbr_val'] = np.concatenate([c['nbr_val'], np.full((1, K), np.nan, dtype=np.float32)])
    g['nbr_len'] = np.concatenate([c['nbr_len'], np.array([K], dtype=np.int32)])
    return g


def dev(c):
    def t(a, dt=None):
        a = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        return a if dt is None else a.to(dt)

    return {'Ub': t(c['Ub']), 'V': t(c['V']), 'u': t(c['u'], torch.int32), 'i': t(c['i'], torch.int32), 'beta_u': t(c['beta_u']),
            'beta_i': t(c['beta_i']), 'nbr_idx': t(c['nbr_idx']), 'nbr_val': t(c['nbr_val']), 'nbr_len': t(c['nbr_len'])}


def launch(d, sc, D=None, N=None, K=None, outs=None):
    """one call of the entry -> (parts [4], dUb, coef, scores) as _Buf views (NaN-filled before the call)"""
    B, D0 = d['Ub'].shape
    N0, K0 = d['i'].shape[1] - 1, d['nbr_idx'].shape[1]
    D, N, K = D0 if D is None else D, N0 if N is None else N, K0 if K is None else K
    outs = outs or (_Buf(1, 4), _Buf(B, D0), _Buf(B, 1 + N0 + K0), _Buf(B, 1 + N0))
    ws = torch.empty(max(int(__import__('importlib').import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib').lib()
                                 .sbr_ultragcn_loss_workspace(B)) // 8, 1), device=DEV, dtype=torch.float64)
    call('sbr_ultragcn_loss_fwd_bwd', d['Ub'].data_ptr(), d['V'].data_ptr(), d['u'].data_ptr(), d['i'].data_ptr(), d['beta_u'].data_ptr(),
         d['beta_i'].data_ptr(), d['nbr_idx'].data_ptr(), d['nbr_val'].data_ptr(), d['nbr_len'].data_ptr(), B, D, N, K, d['beta_u'].numel(),
         d['V'].shape[0], *[float(v) for v in sc], outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr, ws.data_ptr(), 8 * ws.numel(), stream())
    return outs


def scatter(coef, Ub, items, n_items, D, grad=1.0):
    """the item-table gradient by 'sbr_scatter_add_scaled_rows_sorted' into a zeroed NaN-guarded buffer, keys sorted as ops does"""
    keys = torch.from_numpy(np.where(items >= 0, items, n_items).astype(np.int32).reshape(-1)).to(DEV)
    skeys, order = torch.sort(keys, stable=True)
    dst = _Buf(n_items, D, fill=0.)
    g = torch.tensor([grad], device=DEV, dtype=torch.float32)
    call('sbr_scatter_add_scaled_rows_sorted', coef.data_ptr(), Ub.data_ptr(), skeys.data_ptr(), order.data_ptr(), keys.numel(), items.shape[1],
         g.data_ptr(), dst.ptr, n_items, D, stream())
    return dst.check_untouched(what='dV')


@pytest.mark.parametrize('D,B,N,K', CASES)
def test_against_float64_under_the_derived_bound(D, B, N, K):
    c = guarded(R.loss_case(D, B, N, K))
    sc = R.SCALARS
    ref = R.reference(c['Ub'], c['V'][:-1], c['u'], c['i'], c['beta_u'], c['beta_i'][:-1], c['nbr_idx'][:-1], c['nbr_val'][:-1],
                      c['nbr_len'][:-1], sc)
    items = ref['items']
    assert (items < 0).any() and np.abs(ref['scores'][0]).max() > (25 if D > 1 or B > 1 else 0), 'padded slots and large scores are in the case'
    d = dev(c)
    parts, dUb, coef, scores = launch(d, sc)
    got = {'parts': parts.check_untouched(what='parts')[0, :3].numpy(), 'loss': float(parts.host()[0, 3]),
           'dUb': dUb.check_untouched(what='dUb').numpy(), 'coef': coef.check_untouched(what='coef').numpy(),
           'scores': scores.check_untouched(what='scores').numpy()}
    n_items = c['V'].shape[0]
    got['dV'] = scatter(coef.t.contiguous(), d['Ub'], items, n_items, D).numpy()
    assert all(np.isfinite(v).all() for v in got.values()), 'a NaN: a padded slot or the guard row was read'
    assert np.all(got['coef'][items < 0] == 0) and np.all(got['dV'][-1] == 0)
    ref['scores'] = (ref['scores'][0][:, :1 + N], ref['scores'][1][:, :1 + N])
    ref['dV'] = (np.concatenate([ref['dV'][0], np.zeros((1, D))]), np.concatenate([ref['dV'][1], np.zeros((1, D))]))
    worst = {}
    for k in ('parts', 'loss', 'scores', 'coef', 'dUb', 'dV'):
        want, bound = ref[k]
        err = np.abs(np.asarray(got[k], dtype=np.float64) - want)
        ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.)
        worst[k] = float(np.max(ratio))
    print(f'D={D} B={B} N={N} K={K}: error / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, f'{k}: error over the derived bound by a factor of {v:.3f}'
    # two runs, the same bits; the autograd function gives the bits of the direct calls
    again = launch(d, sc)
    for a, b, name in zip((parts, dUb, coef, scores), again, ('parts', 'dUb', 'coef', 'scores')):
        _assert_bits(a.host(), b.host(), f'second run: {name}')
    Ub = d['Ub'].clone().requires_grad_(True)
    V = d['V'].clone().requires_grad_(True)
    loss, three, sco = S().ops.UltraGCNLossFn.apply(Ub, V, d['u'], d['i'], d['beta_u'], d['beta_i'], d['nbr_idx'], d['nbr_val'], d['nbr_len'], *sc)
    loss.backward()
    torch.cuda.synchronize()
    _assert_bits(loss.detach().cpu().reshape(1), parts.host()[0, 3:], 'UltraGCNLossFn: loss')
    _assert_bits(three.cpu(), parts.host()[0, :3], 'UltraGCNLossFn: parts')
    _assert_bits(sco.cpu(), scores.host(), 'UltraGCNLossFn: scores')
    _assert_bits(Ub.grad.cpu(), dUb.host(), 'UltraGCNLossFn: dUb')
    _assert_bits(V.grad.cpu(), torch.from_numpy(got['dV']), 'UltraGCNLossFn: dV')
    assert not three.requires_grad and not sco.requires_grad
    # the item-table gradient in the stated order, by numpy float32
    if B * (1 + N + K) <= ORACLE_MAX_SLOTS:
        for grad in (1.0, 0.75):
            want = R.scatter_ordered32(got['coef'], c['Ub'], items, n_items, grad)
            have = scatter(coef.t.contiguous(), d['Ub'], items, n_items, D, grad)
            _assert_bits(have, torch.from_numpy(want), f'dV against the order oracle, grad = {grad}')


def test_refusals_write_nothing():
    Sm = S()
    c = R.loss_case(8, 3, 2, 4)
    d = dev(c)
    outs = (_Buf(1, 4), _Buf(3, 8), _Buf(3, 7), _Buf(3, 3))
    for kw, text in (({'D': 257}, r'sbr_ultragcn_loss_fwd_bwd: D=257 outside \[1, 256\]'), ({'K': 65}, r'sbr_ultragcn_loss_fwd_bwd: K=65 outside \[1, 64\]'),
                     ({'N': 0}, 'sbr_ultragcn_loss_fwd_bwd: N=0'), ({'D': 0}, 'sbr_ultragcn_loss_fwd_bwd: D=0')):
        with pytest.raises(Sm.SibrarHipError, match=text):
            launch(d, R.SCALARS, outs=outs, **kw)
        for o in outs:
            assert bool(torch.isnan(o.flat).all()), f'{kw}: an output was written'
    wide = torch.zeros(c['V'].shape[0], 16, device=DEV)
    wide[:, :8] = d['V']
    args = (d['u'], d['i'], d['beta_u'], d['beta_i'], d['nbr_idx'], d['nbr_val'], d['nbr_len'], *R.SCALARS)
    with pytest.raises(ValueError, match='UltraGCNLossFn: the item table must be a contiguous float32 matrix'):
        Sm.ops.UltraGCNLossFn.apply(d['Ub'], wide[:, :8], *args)
    with pytest.raises(ValueError, match='UltraGCNLossFn'):
        Sm.ops.UltraGCNLossFn.apply(d['Ub'][:2], d['V'], *args)
    with pytest.raises(Sm.SibrarHipError, match='sbr_ultragcn_loss_fwd_bwd: N=0'):
        Sm.ops.UltraGCNLossFn.apply(d['Ub'], d['V'], d['u'], d['i'][:, :1], *args[2:])
    dst = _Buf(4, 8, fill=0.)
    one = torch.ones(1, device=DEV)
    keys = torch.zeros(6, device=DEV, dtype=torch.int32)
    order = torch.arange(6, device=DEV)
    coef = torch.ones(6, device=DEV)
    for a, text in (((6, 3, one.data_ptr(), dst.ptr, 4, 257), r'D=257 outside \[1, 256\]'), ((6, 4, one.data_ptr(), dst.ptr, 4, 8), '6 slots are no whole number of rows of 4')):
        with pytest.raises(Sm.SibrarHipError, match='sbr_scatter_add_scaled_rows_sorted: ' + text):
            call('sbr_scatter_add_scaled_rows_sorted', coef.data_ptr(), d['Ub'].data_ptr(), keys.data_ptr(), order.data_ptr(), *a, stream())
    assert bool((dst.check_untouched(what='dst') == 0).all())
