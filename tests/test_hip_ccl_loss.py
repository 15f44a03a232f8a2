"""'sbr_ccl_loss_fwd_bwd' (with 'sbr_ccl_loss_workspace') and 'sbr_scatter_add_cos_rows_sorted' (csrc/simplex.hip, ``ops.CCLLossFn``) on the
GPU against float64 under the derived bound of tests/simplex_ref.py (c). Three groups of inputs, all defined there: shapes (both chunk
widths, lane groups below and at the wave, several chunks per lane, one and several rows per wave, a fold of the row partials over one
and two waves), slots and rows (a positive that is its own negative, repeats, indices of -1 and n_items, zero rows on either side) and
the margin (1 on an all-identical table: nothing active, with scores exactly on it; -1: everything active). Per case: scores, parts, dH
and dV through ``CCLLossFn`` inside the bound, the exact sign pattern of both coefficient arrays, the same bits from two runs, the item
table's gradient bit for bit against the numpy float32 order oracle, and no launch counted as nondeterministic in deterministic mode.
The scatter entry on its own on a hand-built sorted key list; the refusals.

Largest error / bound ratios measured on an MI355X (printed by the tests): parts 0.138, scores 0.351, coef_a 0.228, coef_s 0.202, dH 0.101,
dV 0.116."""
from importlib import import_module

import numpy as np
import pytest
import torch

import simplex_ref as R
from hip_testutil import DEV, S, _Buf, _assert_bits, call, stream

pytestmark = pytest.mark.gpu
ORACLE_MAX_SLOTS = 5000                      # the order oracle is a Python loop over the slots


def _t(a, dt=None):
    a = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return a if dt is None else a.to(dt)


def launch(H, V, i32, margin, negw, D=None, N=None, outs=None, eps=R.EPS):
    """one call of the entry -> (parts [3], dH, coef_a, coef_s, scores) as _Buf views (NaN-filled before the call)"""
    B, D0 = H.shape
    N0 = i32.shape[1] - 1
    D, N = D0 if D is None else D, N0 if N is None else N
    outs = outs or (_Buf(1, 3), _Buf(B, D0), _Buf(B, 1 + N0), _Buf(B, 1 + N0), _Buf(B, 1 + N0))
    lib = import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib').lib()
    ws = torch.empty(max(int(lib.sbr_ccl_loss_workspace(B)) // 8, 1), device=DEV, dtype=torch.float64)
    call('sbr_ccl_loss_fwd_bwd', H.data_ptr(), V.data_ptr(), i32.data_ptr(), B, D, N, V.shape[0], float(margin), float(negw), eps, outs[0].ptr,
         outs[1].ptr, outs[2].ptr, outs[3].ptr, outs[4].ptr, ws.data_ptr(), 8 * ws.numel(), stream())
    return outs


def scatter(ca, cs, H, V, keys, slots_per_row, grad=1.0, dst=None):
    """'sbr_scatter_add_cos_rows_sorted' into a NaN-guarded buffer (zeros by default), keys int array [n_slots] sorted as ops does"""
    n_items, D = V.shape
    keys = torch.from_numpy(np.asarray(keys, dtype=np.int32).reshape(-1)).to(DEV)
    skeys, order = torch.sort(keys, stable=True)
    dst = _Buf(n_items, D, fill=0.) if dst is None else dst
    g = torch.tensor([grad], device=DEV, dtype=torch.float32)
    call('sbr_scatter_add_cos_rows_sorted', ca.data_ptr(), cs.data_ptr(), H.data_ptr(), V.data_ptr(), skeys.data_ptr(), order.data_ptr(),
         keys.numel(), slots_per_row, g.data_ptr(), dst.ptr, n_items, D, stream())
    return dst.check_untouched(what='dV')


def check(H32, V32, i, margin, negw, what):
    """everything the issue asks per case -> the worst error / bound ratios"""
    Sm = S()
    ref = R.reference(H32, V32, i, margin, negw)
    H, V, i32 = _t(H32), _t(V32), _t(i, torch.int32)
    n_items, D = V32.shape
    B, C = i.shape
    outs = launch(H, V, i32, margin, negw)
    names = ('parts', 'dH', 'coef_a', 'coef_s', 'scores')
    got = {n: o.check_untouched(what=n).numpy() for n, o in zip(names, outs)}
    got['parts'] = got['parts'][0]
    keys = np.where((i >= 0) & (i < n_items), i, n_items)
    ca, cs = outs[2].t.contiguous(), outs[3].t.contiguous()
    got['dV'] = scatter(ca, cs, H, V, keys, C).numpy()
    assert all(np.isfinite(v).all() for v in got.values()), 'outputs stay finite'
    # the hinge's active set and the clamps, exactly: the sign pattern of both coefficient arrays is the reference's
    for k in ('coef_a', 'coef_s'):
        assert np.array_equal(np.sign(got[k]), np.sign(ref[k][0])), f'{k}: sign pattern'
        assert not np.signbit(got[k][ref['r']['g'] == 0]).any(), f'{k}: +0 in a slot without a gradient'
    outside = (i < 0) | (i >= n_items)
    assert np.all(got['scores'][outside] == 0) and np.all(got['coef_a'][outside] == 0) and np.all(got['coef_s'][outside] == 0)
    worst = R.worst_ratios(got, ref)
    # through the autograd function: the bits of the direct calls, and so inside the bound
    Hg, Vg = H.clone().requires_grad_(True), V.clone().requires_grad_(True)
    prev = Sm.ops.set_deterministic(True)
    try:
        before = Sm.ops.nondeterministic_launches()
        loss, two, sco = Sm.ops.CCLLossFn.apply(Hg, Vg, i32, margin, negw)
        loss.backward()
        torch.cuda.synchronize()
        assert Sm.ops.nondeterministic_launches() == before, 'CCLLossFn took an arrival-order path'
    finally:
        Sm.ops.set_deterministic(prev)
    fn = {'parts': np.concatenate([two.cpu().numpy(), loss.detach().cpu().numpy().reshape(1)]), 'scores': sco.cpu().numpy(),
          'dH': Hg.grad.cpu().numpy(), 'dV': Vg.grad.cpu().numpy()}
    for k, v in R.worst_ratios(fn, ref, keys=tuple(fn)).items():
        worst[k] = max(worst[k], v)
    print(f'{what}: error / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, f'{k}: error over the derived bound by a factor of {v:.3f}'
    assert not two.requires_grad and not sco.requires_grad and tuple(two.shape) == (2,) and tuple(sco.shape) == (B, C)
    for k in fn:
        _assert_bits(torch.from_numpy(fn[k]), torch.from_numpy(got[k]), f'CCLLossFn: {k}')
    # two runs, the same bits
    again = launch(H, V, i32, margin, negw)
    for a, b, n in zip(outs, again, names):
        _assert_bits(a.host(), b.host(), f'second run: {n}')
    _assert_bits(scatter(ca, cs, H, V, keys, C), torch.from_numpy(got['dV']), 'second run: dV')
    # the item table's gradient in the stated order, by numpy float32, onto a table that already holds something
    if B * C <= ORACLE_MAX_SLOTS:
        for grad in (1.0, 0.75):
            start = np.random.default_rng(1).standard_normal(V32.shape).astype(np.float32)
            want = R.scatter_cos32(got['coef_a'], got['coef_s'], H32, V32, i, grad, start)
            have = scatter(ca, cs, H, V, keys, C, grad, _Buf(n_items, D, data=torch.from_numpy(start)))
            _assert_bits(have, torch.from_numpy(want), f'dV against the order oracle, grad = {grad}')
    return worst, got, ref


@pytest.mark.parametrize('D,N,B', R.SHAPE_CASES)
def test_shapes_against_float64_under_the_derived_bound(D, N, B):
    H, V, i, margin, negw = R.shape_case(D, N, B)
    _, got, ref = check(H, V, i, margin, negw, f'D={D} N={N} B={B}')
    if D > 1 and B * N >= 10:
        active = ref['r']['g'][:, 1:] != 0
        assert active.any() and not active.all(), 'the case holds active and inactive negatives'


@pytest.mark.parametrize('kind', R.SLOT_CASES)
def test_slots_and_rows(kind):
    H, V, i, margin, negw = R.slot_case(kind)
    _, got, ref = check(H, V, i, margin, negw, kind)
    if kind == 'zero_rows':
        zero_item, zero_h = ~V[np.where((i >= 0) & (i < len(V)), i, 0)].any(axis=2), ~H.any(axis=1)
        assert np.all(got['coef_s'][zero_item] == 0) and not np.signbit(got['coef_s'][zero_item]).any(), 'the self term of a zero item row is +0'
        assert np.all(got['scores'][zero_item] == 0) and np.all(got['scores'][zero_h] == 0)
        assert (got['coef_a'][zero_item] != 0).any(), 'the zero item row is named by an active slot'
        # dH of a zero H row has no self term: it is the chain over the slots alone
        r = ref['r']
        assert np.array_equal(ref['dH'][0][zero_h], np.einsum('bc,bcd->bd', r['coef_a'], r['Vs'])[zero_h])


def test_the_margin_at_its_ends():
    for name, H, V, i, margin, negw, all_active in R.margin_cases():
        _, got, ref = check(H, V, i, margin, negw, name)
        neg = got['coef_a'][:, 1:]
        assert np.all(neg != 0) if all_active else (np.all(neg == 0) and not np.signbit(neg).any()), name
        if not all_active:
            assert np.all(got['scores'][0] == 1) and got['parts'][1] == 0, 'scores exactly on the margin are not active'


def test_scatter_on_a_hand_built_key_list():
    """6 table rows, 4 batch rows of 5 slots: row 0 of the table is named by nobody, row 1 by one slot, row 3 by all the others that are
    not padded, rows 2, 4 and 5 by nobody; 6 slots carry the sentinel key 6"""
    rng = np.random.default_rng(11)
    n_items, D, B, C = 6, 20, 4, 5
    keys = np.full(B * C, 3, dtype=np.int64)
    keys[7] = 1
    keys[[0, 4, 9, 10, 15, 19]] = n_items
    H32 = rng.standard_normal((B, D)).astype(np.float32)
    V32 = rng.standard_normal((n_items, D)).astype(np.float32)
    ca32, cs32 = rng.standard_normal(B * C).astype(np.float32), rng.standard_normal(B * C).astype(np.float32)
    start = rng.standard_normal((n_items, D)).astype(np.float32)
    idx = keys.reshape(B, C)
    for grad in (1.0, -0.375):
        have = scatter(_t(ca32), _t(cs32), _t(H32), _t(V32), keys, C, grad, _Buf(n_items, D, data=torch.from_numpy(start)))
        want = R.scatter_cos32(ca32, cs32, H32, V32, idx, grad, start)
        _assert_bits(have, torch.from_numpy(want), f'hand-built keys, grad = {grad}')
        _assert_bits(have[[0, 2, 4, 5]], torch.from_numpy(start[[0, 2, 4, 5]]), 'rows that no slot names keep their contents')
        assert not torch.equal(have[1], torch.from_numpy(start[1])) and not torch.equal(have[3], torch.from_numpy(start[3]))
    # float64 of the same sums under the chain's bound
    S64 = np.zeros((n_items, D))
    T64, mag = np.zeros(n_items), np.zeros((n_items, D))
    for pos, j in enumerate(keys):
        if j < n_items:
            S64[j] += float(ca32[pos]) * H32[pos // C].astype(np.float64)
            T64[j] += float(cs32[pos])
            mag[j] += abs(float(ca32[pos])) * np.abs(H32[pos // C]) + abs(float(cs32[pos])) * np.abs(V32[j])
    want64 = start + S64 + T64[:, None] * V32
    have = scatter(_t(ca32), _t(cs32), _t(H32), _t(V32), keys, C, 1.0, _Buf(n_items, D, data=torch.from_numpy(start))).numpy()
    assert np.all(np.abs(have - want64) <= R.SECOND * R.gamma(B * C + 3) * (mag + np.abs(start)))


def test_refusals_write_nothing():
    Sm = S()
    H32, V32, i, margin, negw = R.slot_case('repeats')
    H, V, i32 = _t(H32), _t(V32), _t(i, torch.int32)
    B, D = H32.shape
    C = i.shape[1]
    outs = (_Buf(1, 3), _Buf(B, D), _Buf(B, C), _Buf(B, C), _Buf(B, C))
    for kw, text in (({'D': 257}, r'sbr_ccl_loss_fwd_bwd: D=257 outside \[1, 256\]'), ({'N': 0}, 'sbr_ccl_loss_fwd_bwd: N=0'),
                     ({'D': 0}, 'sbr_ccl_loss_fwd_bwd: D=0'), ({'eps': 0.}, 'sbr_ccl_loss_fwd_bwd: eps=0')):
        with pytest.raises(Sm.SibrarHipError, match=text):
            launch(H, V, i32, margin, negw, outs=outs, **kw)
        for o in outs:
            assert bool(torch.isnan(o.flat).all()), f'{kw}: an output was written'
    wide = torch.zeros(V.shape[0], 2 * D, device=DEV)
    with pytest.raises(ValueError, match='CCLLossFn: the item table must be a contiguous float32 matrix'):
        Sm.ops.CCLLossFn.apply(H, wide[:, :D], i32, margin, negw)
    with pytest.raises(ValueError, match='CCLLossFn'):
        Sm.ops.CCLLossFn.apply(H[:2], V, i32, margin, negw)
    with pytest.raises(Sm.SibrarHipError, match='sbr_ccl_loss_fwd_bwd: N=0'):
        Sm.ops.CCLLossFn.apply(H, V, i32[:, :1], margin, negw)
    dst = _Buf(4, 8, fill=0.)
    one = torch.ones(1, device=DEV)
    keys = torch.zeros(6, device=DEV, dtype=torch.int32)
    order = torch.arange(6, device=DEV)
    coef = torch.ones(6, device=DEV)
    for a, text in (((6, 3, one.data_ptr(), dst.ptr, 4, 257), r'D=257 outside \[1, 256\]'),
                    ((6, 4, one.data_ptr(), dst.ptr, 4, 8), '6 slots are no whole number of rows of 4')):
        with pytest.raises(Sm.SibrarHipError, match='sbr_scatter_add_cos_rows_sorted: ' + text):
            call('sbr_scatter_add_cos_rows_sorted', coef.data_ptr(), coef.data_ptr(), H.data_ptr(), V.data_ptr(), keys.data_ptr(), order.data_ptr(),
                 *a, stream())
    assert bool((dst.check_untouched(what='dst') == 0).all())
