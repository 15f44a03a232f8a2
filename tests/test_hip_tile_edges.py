"""The kernels on the 64 x 64 fp32 tile skeleton (csrc/tile64_f32.h: csrc/proto_cos.hip, csrc/anchor_mix.hip, csrc/cluster_affil.hip)
pinned ELEMENTWISE at the edges of the tile, of the K-chunk and of the register-block count, through the raw entry points, on strided
and shifted tables inside NaN-guarded buffers. tests/tile_edges_cases.py has the covering list of shapes, the inputs, the references and
the restated launch rules; tests/test_tile_edges_cpu.py asserts their preconditions without a GPU. The large-shape, norm-wise tests of
the four families (tests/test_hip_protomf.py, test_hip_protomfs.py, test_hip_acf.py, test_hip_ecf.py) stay as they are.

Per case
  1. placement: the table sits at ld = D + 3, one float off the 16-byte boundary, with NaN between its rows and around it (the weight
     table of ProtoMFs at ldwt = N + 1, ECF's dW at lddw = D + 3); every output and every saved tensor has its own guarded buffer; the
     workspace is NaN throughout. Nothing outside the addressed elements may be written, no input may change, every output is finite.
  2. accuracy, per tensor, in the max norm, with the family's constants (KAPPA = 3, REL_FLOOR = 1e-7, no new one):
         max |gpu - truth| <= KAPPA * max(max |cpu16 - truth|, max |cpu1 - truth|) + REL_FLOOR * max |truth|
     truth = float64, cpu16 / cpu1 = the fp32 torch restatement at 16 threads / 1 thread. Integer outputs (arg-mins, mask bytes) are
     compared exactly. D = 1: every cosine is exactly +-1 and every gradient exactly 0 in every precision, so the criterion asks for
     exact zeros there. Every ratio is printed. Three tensors (ACF's lse and exc, ECF's t at D > 1) are held to a derived
     forward-error bound instead; tests/tile_edges_cases.py has the measured ratios that made it necessary and the derivations.
  3. stride invariance: the same call on a contiguous, aligned table gives the same bits in every output (fixed-order kernels).
The autograd functions of ops are held to the same on a column slice of a wider NaN-filled tensor against its contiguous clone."""
import pytest
import torch

import tile_edges_cases as TC
from hip_testutil import DEV, NAN, _Buf, _assert_bits, _i32, _p, call, stream
from tile_edges_cases import KAPPA, REL_FLOOR, TEMP, W_BATCH, W_EXC, W_INC, W_PROTO, case_id, three

pytestmark = pytest.mark.gpu
I32, U8 = torch.int32, torch.uint8


def S():
    import sibrar_amd
    return sibrar_amd


class Report:
    """the three-way criterion of the family's tests, elementwise (max norm instead of the 2-norm)"""

    def __init__(self, title):
        self.title, self.lines, self.bad, self.worst = title, [], [], {}

    def kappa(self, what, gpu, cpu16, cpu1, truth, bound=None):
        """``bound``: an elementwise forward-error bound that takes the criterion's place (the ratio is still printed)"""
        assert gpu.shape == truth.shape, f'{what}: shape {tuple(gpu.shape)} against {tuple(truth.shape)}'
        assert bool(torch.isfinite(gpu).all()), f'{what}: not finite'
        err = lambda a: float((a.double() - truth.double()).abs().max()) if truth.numel() else 0.0
        e_gpu, e16, e1 = err(gpu), err(cpu16), err(cpu1)
        floor = REL_FLOOR * (float(truth.double().abs().max()) if truth.numel() else 0.0)
        cpu = max(e16, e1)
        ok = e_gpu <= KAPPA * cpu + floor
        ratio = e_gpu / cpu if cpu > 0 else (0.0 if e_gpu == 0 else float('inf'))
        derived = ''
        if bound is not None:
            used = float(((gpu.double() - truth.double()).abs() / bound).max())
            ok = used <= 1.0
            derived = f'  derived bound: {used:.2e} of it used'
        line = f'{what:<16} gpu {e_gpu:.3e}  cpu16 {e16:.3e}  cpu1 {e1:.3e}  ratio {ratio:6.2f}  floor {floor:.2e}{derived}{"" if ok else "  FAIL"}'
        self.lines.append(line)
        self.worst[what] = max(self.worst.get(what, 0.0), ratio)
        if not ok:
            self.bad.append(line)

    def exact(self, what, gpu, truth):
        n = int((gpu != truth).sum())
        self.lines.append(f'{what:<16} exact: {n} of {truth.numel()} differ{"" if n == 0 else "  FAIL"}')
        if n:
            self.bad.append(self.lines[-1])

    def finish(self):
        print(f'\n== {self.title}')
        print('\n'.join(self.lines))
        print(f'largest ratio per tensor [{self.title.split()[0]}]:', {k: round(v, 2) for k, v in self.worst.items()})
        assert not self.bad, f'{self.title}: {len(self.bad)} comparison(s) fail:\n' + '\n'.join(self.bad)


def _compare(title, got, refs, rows=None, bounds=None):
    """every tensor of ``got`` against the references; ``rows``: {name: row selection} for the tensors compared on some rows only;
    ``bounds``: {name: derived elementwise bound} for the tensors of tile_edges_cases's last section"""
    truth, cpu16, cpu1 = refs
    rep = Report(title)
    for k, g in got.items():
        sel = (lambda a: a[rows[k]]) if rows and k in rows else (lambda a: a)
        if g.dtype.is_floating_point:
            rep.kappa(k, sel(g), sel(cpu16[k]), sel(cpu1[k]), sel(truth[k]), sel(bounds[k]) if bounds and k in bounds else None)
        else:
            rep.exact(k, sel(g), sel(truth[k]))
    rep.finish()


def _same_bits(a, b, what):
    assert list(a) == list(b)
    for k in a:
        if a[k].dtype.is_floating_point:
            _assert_bits(a[k], b[k], f'{what} {k}: strided against contiguous')
        else:
            assert torch.equal(a[k], b[k]), f'{what} {k}: strided against contiguous'


def _table(t, strided, cols_extra=3, off=1):
    """a read-only table: ld = cols + 3 and one float off the 16-byte boundary, or contiguous and aligned"""
    n, d = t.shape
    return _Buf(n, d, ld=d + cols_extra, off=off, data=t) if strided else _Buf(n, d, data=t)


def _ws(entry, R, D, N, backward):
    """(the workspace ``entry`` asks for, NaN in every float and double of it; its size) — the size is the restated rule's"""
    n = int(getattr(S().lib(), entry)(R, D, N, 1 if backward else 0))
    assert n == TC.ws_bytes(entry, R, D, N, backward), f'{entry}{(R, D, N, backward)}: {n} bytes, the restated rule gives another size'
    return torch.full((max(n, 16),), 0xFF, dtype=U8, device=DEV), n


def _scalar(v):
    return torch.tensor([v], dtype=torch.float32, device=DEV)


VECTORS = ('row_best', 'col_best_val', 'col_best_row', 'proto_loss', 'batch_loss', 'lse', 'q', 'dinc', 'exc', 'inc')


def _collect(outs, inputs):
    """check every guard band, every input for change; -> {name: host tensor}"""
    for name, (buf, data) in inputs.items():
        assert torch.equal(buf.check_untouched(what=name), data), f'{name}: an input changed'
    got = {}
    for name, buf in outs.items():
        h = buf.check_untouched(what=name)
        got[name] = h.reshape(-1) if name in VECTORS else h.clone()
    return got


# ---- ProtoMF -----------------------------------------------------------------------------------------------------------------------------
def _run_sim(inp, strided, fwd_only):
    (R, P), D = inp['G'].shape, inp['table'].shape[1]
    W, Pb, rows = _table(inp['table'], strided), _Buf(P, D, data=inp['protos']), None if inp['rows'] is None else _i32(inp['rows'])
    o = dict(sim=_Buf(R, P), cos_raw=_Buf(R, P), row_stat=_Buf(R, 2), proto_stat=_Buf(P, 2), row_best=_Buf(R, 1, dtype=I32),
             col_best_val=_Buf(P, 1), col_best_row=_Buf(P, 1, dtype=I32), proto_loss=_Buf(1, 1), batch_loss=_Buf(1, 1))
    ws, n = _ws('sbr_proto_sim_workspace', R, D, P, False)
    call('sbr_proto_sim_fwd', W.ptr, W.ld, _p(rows), R, D, Pb.ptr, P, o['sim'].ptr, o['cos_raw'].ptr, o['row_stat'].ptr, o['proto_stat'].ptr,
         o['row_best'].ptr, o['col_best_val'].ptr, o['col_best_row'].ptr, o['proto_loss'].ptr, o['batch_loss'].ptr, _p(ws), n, stream())
    ev = _Buf(R, P)                                     # the evaluation form: no arg-mins, no losses, nothing saved
    ws2, n2 = _ws('sbr_proto_sim_workspace', R, D, P, False)
    call('sbr_proto_sim_fwd', W.ptr, W.ld, _p(rows), R, D, Pb.ptr, P, ev.ptr, None, None, None, None, None, None, None, None, _p(ws2), n2, stream())
    _assert_bits(ev.check_untouched(what='evaluation sim'), o['sim'].host(), 'the evaluation form against the training form')
    inputs = dict(table=(W, inp['table']), protos=(Pb, inp['protos']))
    if not fwd_only:
        G = _Buf(R, P, data=inp['G'])
        o.update(dE=_Buf(R, D), dP=_Buf(P, D))
        wsb, nb = _ws('sbr_proto_sim_workspace', R, D, P, True)
        g_proto, g_batch = _scalar(W_PROTO), _scalar(W_BATCH)
        call('sbr_proto_sim_bwd', G.ptr, _p(g_proto), _p(g_batch), W.ptr, W.ld, _p(rows), R, D, Pb.ptr, P, o['cos_raw'].ptr,
             o['row_stat'].ptr, o['proto_stat'].ptr, o['row_best'].ptr, o['col_best_row'].ptr, o['dE'].ptr, o['dP'].ptr, _p(wsb), nb, stream())
        inputs['G'] = (G, inp['G'])
    return _collect(o, inputs)


@pytest.mark.parametrize('case', TC.SIM_CASES, ids=case_id)
def test_proto_sim_entry_points_elementwise(case):
    """sbr_proto_sim_fwd (training and evaluation form) and sbr_proto_sim_bwd: sim, cos_raw, both stats, the arg-mins (exact), the column
    minimum, both losses, dE, dP"""
    R, D, P, lookup, fwd_only = case
    inp = TC.sim_inputs(R, D, P, lookup)
    TC.sim_precondition(inp)
    if (R, D, P) == TC.REACH_FWD:
        assert TC.tiles(R) > TC.t64_wgs(R, TC.PS_MAX_WG), 'the grid-stride loop of ps_fwd_kernel is not reached'
    a, b = _run_sim(inp, True, fwd_only), _run_sim(inp, False, fwd_only)
    _same_bits(a, b, 'proto_sim')
    _compare(f'proto_sim R={R} D={D} P={P} lookup={lookup}', a, three(lambda dt: TC.sim_ref(inp, dt)))


# ---- ProtoMFs ----------------------------------------------------------------------------------------------------------------------------
def _run_score(inp, strided, fwd_only):
    D, P = inp['table'].shape[1], inp['protos'].shape[0]
    R = inp['G'].shape[0]
    score = inp['wt'] is not None
    fan = inp['G'].shape[1] if score else 1
    W, Pb, rows = _table(inp['table'], strided), _Buf(P, D, data=inp['protos']), None if inp['rows'] is None else _i32(inp['rows'])
    Wt = _table(inp['wt'], strided, cols_extra=1, off=2) if score else None
    widx = _i32(inp['widx']) if score and inp['widx'] is not None else None
    o = dict(cos_raw=_Buf(R, P), row_stat=_Buf(R, 2), proto_stat=_Buf(P, 2))
    o.update(out=_Buf(R, fan)) if score else o.update(cos=_Buf(R, P))
    ws, n = _ws('sbr_proto_score_workspace', R, D, P, False)
    call('sbr_proto_score_fwd', W.ptr, W.ld, _p(rows), R, D, Pb.ptr, P, Wt.ptr if score else None, Wt.ld if score else 0, _p(widx), fan,
         None if score else o['cos'].ptr, o['out'].ptr if score else None, o['cos_raw'].ptr, o['row_stat'].ptr, o['proto_stat'].ptr, _p(ws), n,
         stream())
    inputs = dict(table=(W, inp['table']), protos=(Pb, inp['protos']))
    if score:
        inputs['weights'] = (Wt, inp['wt'])
    if not fwd_only:
        G = _Buf(*inp['G'].shape, data=inp['G'])
        o.update(dE=_Buf(R, D), dP=_Buf(P, D))
        if score:
            o.update(dWrows=_Buf(R * fan, P))
        wsb, nb = _ws('sbr_proto_score_workspace', R, D, P, True)
        call('sbr_proto_score_bwd', G.ptr, W.ptr, W.ld, _p(rows), R, D, Pb.ptr, P, Wt.ptr if score else None, Wt.ld if score else 0, _p(widx),
             fan, o['cos_raw'].ptr, o['row_stat'].ptr, o['proto_stat'].ptr, o['dE'].ptr, o['dP'].ptr, o['dWrows'].ptr if score else None,
             _p(wsb), nb, stream())
        inputs['G'] = (G, inp['G'])
    got = _collect(o, inputs)
    return got


@pytest.mark.parametrize('case', TC.SCORE_CASES, ids=case_id)
def test_proto_score_entry_points_elementwise(case):
    """sbr_proto_score_fwd / _bwd in the cosine form (Wt == NULL) and in the score form with widx given and NULL, fan in {1, 3}: cos or
    out, cos_raw, both stats, dE, dP, dWrows"""
    R, D, P, fan, with_widx, lookup, fwd_only = case
    inp = TC.score_inputs(R, D, P, fan, with_widx, lookup)
    if not fwd_only:
        TC.score_precondition(inp)
    if R == TC.REACH_FWD_SCORE[0]:
        assert TC.tiles(R) > TC.t64_wgs(R, TC.PC_MAX_WG), 'the grid-stride loop of pq_fwd_kernel is not reached'
    a, b = _run_score(inp, True, fwd_only), _run_score(inp, False, fwd_only)
    _same_bits(a, b, 'proto_score')
    refs = three(lambda dt: TC.score_ref(inp, dt))
    _compare(f'proto_score R={R} D={D} P={P} fan={fan} widx={with_widx} lookup={lookup}', a, refs)


# ---- ACF ---------------------------------------------------------------------------------------------------------------------------------
def _run_anchor(inp, strided, loss, fwd_only):
    (R, D), K = inp['G'].shape, inp['anchors'].shape[0]
    W, A, rows = _table(inp['table'], strided), _Buf(K, D, data=inp['anchors']), None if inp['rows'] is None else _i32(inp['rows'])
    o = dict(r=_Buf(R, D), c=_Buf(R, K))
    ws, n = None, 0
    if loss:
        o.update(lse=_Buf(R, 1), q=_Buf(K, 1), dinc=_Buf(K, 1), exc=_Buf(1, 1), inc=_Buf(1, 1))
        ws, n = _ws('sbr_anchor_mix_workspace', R, D, K, False)
    lo = lambda k: o[k].ptr if loss else None
    call('sbr_anchor_mix_fwd', W.ptr, W.ld, _p(rows), R, D, A.ptr, K, o['r'].ptr, o['c'].ptr, lo('lse'), lo('q'), lo('dinc'), lo('exc'), lo('inc'),
         _p(ws), n, stream())
    inputs = dict(table=(W, inp['table']), anchors=(A, inp['anchors']))
    if not fwd_only:
        G = _Buf(R, D, data=inp['G'])
        o.update(dE=_Buf(R, D), dA=_Buf(K, D))
        wsb, nb = _ws('sbr_anchor_mix_workspace', R, D, K, True)
        g_exc, g_inc = (_scalar(W_EXC), _scalar(W_INC)) if loss else (None, None)
        call('sbr_anchor_mix_bwd', G.ptr, _p(g_exc), _p(g_inc), W.ptr, W.ld, _p(rows), R, D,
             A.ptr, K, o['c'].ptr, lo('lse'), lo('dinc'), o['dE'].ptr, o['dA'].ptr, _p(wsb), nb, stream())
        inputs['G'] = (G, inp['G'])
    return _collect(o, inputs)


@pytest.mark.parametrize('case', TC.ANCHOR_CASES, ids=case_id)
def test_anchor_mix_entry_points_elementwise(case):
    """sbr_anchor_mix_fwd / _bwd with and without the loss outputs: r, c, lse, q, d inc / d c, both losses, dE, dA"""
    R, D, K, loss, lookup, fwd_only = case
    inp = TC.anchor_inputs(R, D, K, lookup)
    TC.anchor_precondition(inp)
    if (R, D, K) == TC.REACH_FWD:
        assert TC.tiles(R) > TC.t64_wgs(R), 'the grid-stride loop of am_fwd_kernel is not reached'
    if (R, D, K) == TC.REACH_BWD:
        splits = int(S().lib().sbr_anchor_mix_workspace(R, D, K, 1)) // (K * D * 4)
        assert splits == TC.am_splits(R, D, K) < TC.tiles(R), 'no workgroup of am_bwd_kernel owns a second tile'
    a, b = _run_anchor(inp, True, loss, fwd_only), _run_anchor(inp, False, loss, fwd_only)
    _same_bits(a, b, 'anchor_mix')
    _compare(f'anchor_mix R={R} D={D} K={K} loss={loss} lookup={lookup}', a, three(lambda dt: TC.anchor_ref(inp, dt, loss)),
             bounds=TC.anchor_loss_bounds(inp) if loss else None)


# ---- ECF ---------------------------------------------------------------------------------------------------------------------------------
def _run_cluster(inp, strided, fwd_only):
    (R, C), D, top = inp['G'].shape, inp['W'].shape[1], inp['top']
    W, Cl = _table(inp['W'], strided), _Buf(C, D, data=inp['Cl'])
    o = dict(t=_Buf(R, C), x=_Buf(R, C), row_state=_Buf(R, 4), mask=_Buf(R, (C + 3) // 4, dtype=U8))
    ws, n = _ws('sbr_cluster_affil_workspace', R, D, C, False)
    call('sbr_cluster_affil_fwd', W.ptr, W.ld, Cl.ptr, None, R, D, C, top, TEMP, o['t'].ptr, o['x'].ptr, o['row_state'].ptr, o['mask'].ptr, _p(ws),
         n, stream())
    inputs = dict(table=(W, inp['W']), clusters=(Cl, inp['Cl']))
    if not fwd_only:
        G, Gt = _Buf(R, C, data=inp['G']), _Buf(R, C, data=inp['Gt'])
        o.update(dW=_Buf(R, D, ld=D + 3, off=1) if strided else _Buf(R, D), dCl=_Buf(C, D))
        wsb, nb = _ws('sbr_cluster_affil_workspace', R, D, C, True)
        call('sbr_cluster_affil_bwd', G.ptr, Gt.ptr, W.ptr, W.ld, Cl.ptr, o['t'].ptr, R, D, C, TEMP, o['row_state'].ptr, o['mask'].ptr, o['dW'].ptr,
             o['dW'].ld, o['dCl'].ptr, None, _p(wsb), nb, stream())
        inputs.update(G=(G, inp['G']), Gt=(Gt, inp['Gt']))
    return _collect(o, inputs)


@pytest.mark.parametrize('case', TC.CLUSTER_CASES, ids=case_id)
def test_cluster_affil_cosine_form_elementwise(case):
    """sbr_cluster_affil_fwd / _bwd, cosine form, top in {1, a middle value, C}: t, x, the row state, the mask bytes (exact), dW at
    lddw = D + 3, dCl. The near-tie share is asserted first; the rows left out carry no upstream gradient."""
    R, D, C, top, fwd_only = case
    inp = TC.cluster_inputs(R, D, C, top)
    print(f'\nnear-tie rows left out at {case}: {TC.cluster_precondition(inp):.4f}')
    if (R, D, C) == TC.REACH_FWD:
        assert TC.tiles(R) > TC.t64_wgs(R), 'the grid-stride loop of ca_fwd_cos_kernel is not reached'
    if (R, D, C) == TC.REACH_BWD:
        splits = (int(S().lib().sbr_cluster_affil_workspace(R, D, C, 1)) - 2 * TC.T64_MAX_N * 4) // (C * (D + 1) * 4)
        assert splits == TC.ca_splits(R, D, C) < TC.tiles(R), 'no workgroup of ca_bwd_cos_kernel owns a second tile'
    a, b = _run_cluster(inp, True, fwd_only), _run_cluster(inp, False, fwd_only)
    _same_bits(a, b, 'cluster_affil')
    keep = inp['keep']
    assert bool(((a['x'] != 0).sum(dim=1) == top).all()), 'exactly `top` entries of a row are on the mask'
    _compare(f'cluster_affil cosine form R={R} D={D} C={C} top={top}', a, three(lambda dt: TC.cluster_ref(inp, dt)),
             rows=dict(t=keep, x=keep, mask=keep), bounds=dict(t=TC.cluster_t_bound(inp)) if D > 1 else None)


@pytest.mark.parametrize('case', TC.CLUSTER_CASES, ids=case_id)
def test_cluster_affil_logit_form_elementwise(case):
    """the logit form on N(0, 2) logits: x, the row state, the mask bytes (exact: both sides read the same fp32 values), dt"""
    R, _, C, top, fwd_only = case
    inp = TC.logit_inputs(R, C, top)
    TC.logit_precondition(inp)
    T = _Buf(R, C, data=inp['t'])
    o = dict(x=_Buf(R, C), row_state=_Buf(R, 4), mask=_Buf(R, (C + 3) // 4, dtype=U8))
    call('sbr_cluster_affil_fwd', None, 0, None, T.ptr, R, 0, C, top, TEMP, None, o['x'].ptr, o['row_state'].ptr, o['mask'].ptr, None, 0, stream())
    inputs = dict(logits=(T, inp['t']))
    if not fwd_only:
        G = _Buf(R, C, data=inp['G'])
        o.update(dt=_Buf(R, C))
        call('sbr_cluster_affil_bwd', G.ptr, None, None, 0, None, T.ptr, R, 0, C, TEMP, o['row_state'].ptr, o['mask'].ptr, None, 0, None,
             o['dt'].ptr, None, 0, stream())
        inputs['G'] = (G, inp['G'])
    _compare(f'cluster_affil logit form R={R} C={C} top={top}', _collect(o, inputs), three(lambda dt: TC.logit_ref(inp, dt)))


# ---- the autograd functions on a column slice of a wider tensor -----------------------------------------------------------------------------
def _sliced(t, left=2, right=3):
    """(big [n, left + cols + right] on the device, NaN outside the slice; the slice as a leaf that shares big's storage)"""
    big = torch.full((t.shape[0], left + t.shape[1] + right), NAN)
    big[:, left:left + t.shape[1]] = t
    big = big.to(DEV)
    view = big[:, left:left + t.shape[1]].detach().requires_grad_(True)
    assert view.data_ptr() == big.data_ptr() + 4 * left and view.stride(0) == big.shape[1]
    return big, view


def _slice_untouched(big, t, left=2):
    host = big.cpu()
    inside = torch.zeros(host.shape, dtype=torch.bool)
    inside[:, left:left + t.shape[1]] = True
    assert bool(torch.isnan(host[~inside]).all()), 'the wider tensor was written outside the slice'
    _assert_bits(host[:, left:left + t.shape[1]], t, 'the slice itself changed')


def _both(fn, sliced, plain, what):
    """fn(table) -> (outputs, leaves): the same bits from the slice and from its contiguous clone, forward and backward"""
    out_s, leaves_s = fn(sliced)
    out_p, leaves_p = fn(plain)
    torch.cuda.synchronize()
    for n, (s, p) in enumerate(zip(out_s, out_p)):
        _assert_bits(s.detach().cpu(), p.detach().cpu(), f'{what}: output {n}')
    for n, (s, p) in enumerate(zip(leaves_s, leaves_p)):
        assert bool(torch.isfinite(s.grad).all())
        _assert_bits(s.grad.cpu(), p.grad.cpu(), f'{what}: gradient {n}')


@pytest.mark.parametrize('R,D,N', TC.OPS_SHAPES)
def test_ops_on_a_column_slice_give_the_bits_of_the_contiguous_clone(R, D, N):
    """ProtoSimFn, ProtoCosFn, ProtoScoreFn (the weights a slice too), AnchorMixFn and ClusterAffilFn on ``big[:, 2:2 + D]``: ld = D + 5,
    rows 8 bytes off the 16-byte boundary, NaN on both sides of every row"""
    ops = S().ops
    plain = lambda t: t.detach().to(DEV).contiguous().requires_grad_(True)
    dev = lambda t: t.to(DEV)

    inp = TC.sim_inputs(R, D, N, True)
    big, view = _sliced(inp['table'])

    def sim(table):
        p = plain(inp['protos'])
        s, pl, bl = ops.ProtoSimFn.apply(table, dev(inp['rows']), p)
        ((s * dev(inp['G'])).sum() + W_PROTO * pl + W_BATCH * bl).backward()
        return (s, pl, bl), (table, p)
    _both(sim, view, plain(inp['table']), 'ProtoSimFn')
    _slice_untouched(big, inp['table'])

    inp = TC.score_inputs(R, D, N, 0, False, True)
    big, view = _sliced(inp['table'])

    def cos(table):
        p = plain(inp['protos'])
        c = ops.ProtoCosFn.apply(table, dev(inp['rows']), p)
        (c * dev(inp['G'])).sum().backward()
        return (c,), (table, p)
    _both(cos, view, plain(inp['table']), 'ProtoCosFn')
    _slice_untouched(big, inp['table'])

    inp = TC.score_inputs(R, D, N, 3, True, True)
    big, view = _sliced(inp['table'])
    wbig, wview = _sliced(inp['wt'], 1, 2)

    def score(tw):
        table, w = tw
        p = plain(inp['protos'])
        o = ops.ProtoScoreFn.apply(table, dev(inp['rows']), p, w, dev(inp['widx']), 3)
        (o * dev(inp['G'])).sum().backward()
        return (o,), (table, p, w)
    _both(score, (view, wview), (plain(inp['table']), plain(inp['wt'])), 'ProtoScoreFn')
    _slice_untouched(big, inp['table'])
    _slice_untouched(wbig, inp['wt'], 1)

    inp = TC.anchor_inputs(R, D, N, True)
    big, view = _sliced(inp['table'])

    def mix(table):
        a = plain(inp['anchors'])
        r, c, exc, inc = ops.AnchorMixFn.apply(table, dev(inp['rows']), a, True)
        ((r * dev(inp['G'])).sum() + W_EXC * exc + W_INC * inc).backward()
        return (r, c, exc, inc), (table, a)
    _both(mix, view, plain(inp['table']), 'AnchorMixFn')
    _slice_untouched(big, inp['table'])

    inp = TC.cluster_inputs(R, D, N, 20)
    big, view = _sliced(inp['W'])

    def affil(table):
        c = plain(inp['Cl'])
        t, x = ops.ClusterAffilFn.apply(table, c, None, 20, TEMP)
        ((x * dev(inp['G'])).sum() + (t * dev(inp['Gt'])).sum()).backward()
        return (t, x), (table, c)
    _both(affil, view, plain(inp['W']), 'ClusterAffilFn')
    _slice_untouched(big, inp['W'])
