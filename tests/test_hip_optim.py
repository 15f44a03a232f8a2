"""GPU: the optimizer kernels (csrc/optim.hip) through the C ABI against the float64 update rules of tests/optim_ref.py, one step at a
time from a given fp32 state, under the derived per-step bounds of that module (its header has the derivation; test_optim_refs_cpu.py
shows on the CPU that an fp32 restatement passes them on every input set generated here and that the listed wrong kernels do not).

Conventions of this file
  * Every comparison is ONE step: in a multi-step case the kernel's own output state goes back into the reference, so the bound is a
    per-step bound and drift plays no part. p, both moments and Adagrad's state_sum are compared, each with its own bound.
  * Operands live in NaN-filled buffers (hip_testutil._Buf): a write outside [0, n) fails the test, a read outside poisons the result.
  * adamw_kernel takes 16-byte accesses iff n % 4 == 0 and p | g | m | v is 16-byte aligned, else its element loop: every n % 4 == 0 runs
    aligned, with all four pointers 4 bytes off and with each single one off; all runs must agree bit for bit.
  * grid_for caps a launch at 8,192 workgroups of 256 threads: the two sizes of test_behind_the_launch_cap make the element loop and
    the 16-byte path take a second trip of their grid-stride loops.
  * State: m and v log-uniform over many decades with exact zeros and denormals (v down to 1e-38 and below), g with exact zeros, -0.0
    and magnitudes 1e-6 .. 1e2 (``state``); the hyper-parameter sets HYPERS cover every value once, not the product.
Every check prints its largest error / bound ratio (pytest -s shows them)."""
import numpy as np
import pytest
import torch

import optim_ref as O
from hip_testutil import DEV, GUARD, NAN, S, _L, _assert_bits, _bits, _Buf, _i32, _i64, call, stream

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 255, 256, 257, 1024, 4100]
N_CAP_ELEMENT = 8192 * 256 + 259                     # element loop: 259 elements behind the first trip of the capped grid
N_CAP_QUAD = 4 * (8192 * 256 + 64)                   # 16-byte path: 64 quads behind it (33.6 MB per buffer)
# (lr, wd, b1, b2, eps, step)
HYPERS = [(1e-3, 1e-2, 0.9, 0.999, 1e-8, 1), (1e-5, 0.0, 0.0, 0.9, 1e-12, 2), (1e-1, 0.3, 0.5, 0.99, 1e-3, 10),
          (1e-2, 1e-2, 0.99, 0.999, 1e-8, 1000), (3e-4, 0.3, 0.9, 0.99, 1e-12, 10 ** 6), (1e-2, 0.0, 0.99, 0.9, 1e-3, 1),
          (0.0, 0.3, 0.9, 0.999, 1e-8, 2), (1e-3, 1e-2, 0.5, 0.999, 1e-8, 10)]
# (lr, eps, wd)
HYPERS_ADAGRAD = [(1e-2, 1e-10, 1e-2), (1e-5, 1e-8, 0.0), (1e-1, 1e-3, 0.3), (0.0, 1e-10, 0.3)]
N_STEPS = 3                                          # steps of a multi-step case (the state is fed back)


# ---- the case generator (also imported by tests/test_optim_refs_cpu.py) ---------------------------------------------------------
def _loguniform(n, lo, hi, g):
    return torch.pow(10.0, torch.rand(n, generator=g, dtype=torch.float64) * (hi - lo) + lo)


def _sign(n, g):
    return torch.randint(0, 2, (n,), generator=g).double() * 2 - 1


def state(n, seed):
    """-> fp32 (p, g, m, v) of n elements; v doubles as Adagrad's state_sum"""
    gen = torch.Generator().manual_seed(seed)
    idx = torch.randperm(n, generator=gen)
    p = (_sign(n, gen) * _loguniform(n, -4, 1, gen)).float()
    m = (_sign(n, gen) * _loguniform(n, -12, 0, gen)).float()
    v = _loguniform(n, -38, 0, gen).float()
    g = (_sign(n, gen) * _loguniform(n, -6, 2, gen)).float()
    # a tenth each, at positions that do not line up between the tensors: exact zeros, denormals, -0.0
    k = n // 10
    p[idx[:k]] = 0.0
    m[idx[k // 2: k // 2 + k]] = 0.0
    m[idx[2 * k: 3 * k]] = (_sign(k, gen) * _loguniform(k, -45, -39, gen)).float()[: len(idx[2 * k: 3 * k])]
    v[idx[k: 2 * k]] = 0.0
    v[idx[3 * k: 4 * k]] = _loguniform(k, -45, -39, gen).float()[: len(idx[3 * k: 4 * k])]
    g[idx[k + k // 2: 3 * k]] = 0.0
    g[idx[4 * k: 5 * k]] = -0.0
    return p, g, m, v


def next_gradient(n, seed, t):
    return state(n, seed * 1000 + t)[1]


def dense_cases():
    """every (optimizer, n, hyper-parameters, seed, steps) the dense tests below run; optimizer 0 AdamW, 1 Adam, 2 Adagrad"""
    cases = []
    for opt in (0, 1, 2):
        hy = HYPERS_ADAGRAD if opt == 2 else HYPERS
        for i, n in enumerate(SIZES):
            cases.append((opt, n, hy[(i + opt) % len(hy)], 100 * opt + i, 1))
        for j, h in enumerate(hy):
            cases.append((opt, 1028, h, 100 * opt + 50 + j, N_STEPS))
    cases += [(0, N_CAP_ELEMENT, HYPERS[0], 901, 1), (1, N_CAP_ELEMENT, HYPERS[2], 902, 1), (2, N_CAP_ELEMENT, HYPERS_ADAGRAD[0], 903, 1),
              (1, N_CAP_QUAD, HYPERS[3], 904, 1), (0, N_CAP_QUAD, HYPERS[4], 905, 1)]
    return cases


def rule(opt, p, g, m, v, h, t=0):
    """one step of the float64 rule -> (outputs, bounds) in the order (p, m, v) or (p, state_sum); t: steps already taken in this case"""
    if opt == 2:
        return O.adagrad_ref(p, g, v, h[0], h[1], h[2])
    lr, wd, b1, b2, eps, step = h
    return O.adam_ref(opt, p, g, m, v, lr, b1, b2, eps, wd, step + t)


NAMES = {0: ('p', 'm', 'v'), 1: ('p', 'm', 'v'), 2: ('p', 'state_sum')}


# ---- running a kernel ------------------------------------------------------------------------------------------------------------
def _bufs(tensors, offs=(0, 0, 0, 0)):
    out = []
    for t, off in zip(tensors, offs):
        b = _Buf(1, t.numel(), off=off, data=t.view(1, -1))
        assert b.ptr % 16 == 4 * off
        out.append(b)
    return out


def _launch(opt, zero, P, G, M, V, n, h, t=0, copy=(None, None, 0)):
    if opt == 2:
        call('sbr_adagrad_step', P.ptr, G.ptr, V.ptr, n, h[0], h[1], h[2], stream())
        return
    lr, wd, b1, b2, eps, step = h
    if zero:
        call('sbr_adam_step_zero_grad', opt, P.ptr, G.ptr, M.ptr, V.ptr, n, lr, b1, b2, eps, wd, step + t, copy[0], copy[1], copy[2], stream())
    else:
        call('sbr_adam_step', opt, P.ptr, G.ptr, M.ptr, V.ptr, n, lr, b1, b2, eps, wd, step + t, stream())


def _one_step(opt, zero, tensors, h, t=0, offs=(0, 0, 0, 0), what=''):
    """one launch on (p, g, m, v) -> the fp32 outputs (p, m, v) / (p, state_sum) on the host, compared with the float64 rule; checks
    the guards and the gradient buffer"""
    p, g, m, v = tensors
    n = p.numel()
    P, G, M, V = _bufs(tensors, offs)
    _launch(opt, zero, P, G, M, V, n, h, t)
    got = [b.check_untouched(None, f'{what} {nm}')[0] for b, nm in zip((P, G, M, V), 'pgmv')]
    if opt != 2 and zero:
        assert not bool(_bits(got[1]).any()), f'{what}: the gradient is not +0 in every bit'
    else:
        _assert_bits(got[1], g, f'{what}: the gradient buffer changed')
    if opt == 2:
        _assert_bits(got[2], m, f'{what}: adagrad touched a buffer it was not given')
    outs = (got[0], got[3]) if opt == 2 else (got[0], got[2], got[3])
    refs, bounds = rule(opt, p, g, m, v, h, t)
    for o, r, b, nm in zip(outs, refs, bounds, NAMES[opt]):
        ratio = O.check_bound(o, r, b, f'{what} {nm}')
        print(f'ratio {nm} {ratio:.3f} {what}')
    return outs


def _entries(opt):
    return (False,) if opt == 2 else (False, True)


# ---- dense kernels: sizes, alignments, paths -------------------------------------------------------------------------------------
@pytest.mark.parametrize('opt,n,h,seed,steps', [c for c in dense_cases() if c[4] == 1 and c[1] <= 4100])
def test_dense_step_sizes_and_paths(opt, n, h, seed, steps):
    """sbr_adam_step, sbr_adam_step_zero_grad (AdamW, Adam) and sbr_adagrad_step at every size: p, m, v / state_sum within the
    per-step bound of the float64 rule; 16-byte path (aligned, n % 4 == 0) and element loop (all four pointers, or any single one,
    4 bytes off) bit-identical on the same data; nothing outside [0, n) written; the gradient left alone resp. +0 in every bit."""
    tensors = state(n, seed)
    layouts = [(0, 0, 0, 0)]
    if n % 4 == 0:
        layouts += [(1, 1, 1, 1), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)]
    first = None
    for zero in _entries(opt):
        for offs in layouts:
            outs = _one_step(opt, zero, tensors, h, offs=offs, what=f'opt {opt} zero {zero} n {n} offs {offs}')
            if first is None:
                first = outs
            for a, b, nm in zip(outs, first, NAMES[opt]):
                _assert_bits(a, b, f'{nm}: offs {offs}, zero {zero} differs from the first run')


@pytest.mark.parametrize('opt,n,h,seed,steps', [c for c in dense_cases() if c[4] > 1])
def test_dense_step_hyper_parameters(opt, n, h, seed, steps):
    """Every hyper-parameter set over N_STEPS steps at n = 1028 (16-byte path, five workgroups), the kernel's own output state fed back
    into the reference; with lr = 0 the parameters change through AdamW's decay only and m, v move as always."""
    p, g, m, v = state(n, seed)
    zero = opt != 2 and seed % 2 == 1
    for t in range(steps):
        outs = _one_step(opt, zero, (p, g, m, v), h, t, what=f'opt {opt} h {h} step +{t}')
        if h[0] == 0.0:
            _assert_bits(outs[0], p, 'lr = 0: the parameters moved')
        p = outs[0]
        m, v = (m, outs[1]) if opt == 2 else (outs[1], outs[2])
        g = next_gradient(n, seed, t)


@pytest.mark.parametrize('opt,n,h,seed,steps', [c for c in dense_cases() if c[1] > 4100])
def test_behind_the_launch_cap(opt, n, h, seed, steps):
    """The grid-stride tail behind grid_for's cap of 8,192 workgroups: the element loop at 8192 * 256 + 259 elements, the 16-byte path
    at 4 * (8192 * 256 + 64). Every element up to the last is updated (the bound holds on all of them; the second moment / state_sum of
    the tail moved) and the guards behind the last element are intact."""
    tensors = state(n, seed)
    zero = opt != 2 and seed % 2 == 0
    outs = _one_step(opt, zero, tensors, h, what=f'opt {opt} n {n}')
    tail = slice(8192 * 256 * (4 if n % 4 == 0 else 1), n)
    moved = _bits(outs[-1][tail]) != _bits(tensors[3][tail])
    assert int(moved.sum()) > 0.5 * moved.numel(), 'the elements behind the first trip of the grid were not updated'


@pytest.mark.parametrize('opt', [0, 1, 2])
@pytest.mark.parametrize('off', [0, 1])
def test_non_finite_gradients_stay_in_their_element(opt, off):
    """g = inf, -inf and NaN in single elements of different 16-byte quads (aligned: 16-byte path; 4 bytes off: element loop): those
    elements come out in the class the float64 rule gives (NaN parameter; inf / NaN moments), their neighbours within the bound."""
    n = 16
    p, g, m, v = state(n, 77 + opt)
    g[1], g[6], g[11] = float('inf'), float('-inf'), NAN
    h = HYPERS_ADAGRAD[0] if opt == 2 else HYPERS[0]
    for zero in _entries(opt):
        outs = _one_step(opt, zero, (p, g, m, v), h, offs=(off,) * 4, what=f'opt {opt} non-finite g, off {off}')
        bad = torch.zeros(n, dtype=torch.bool)
        bad[[1, 6, 11]] = True
        for o in outs:
            assert bool(torch.isfinite(o[~bad]).all()) and not bool(torch.isfinite(o[bad]).any())


@pytest.mark.parametrize('n', [3, 1000])
@pytest.mark.parametrize('copy_n', [0, 1, 3, 256])
def test_zero_grad_launch_copies_exactly_copy_n_doubles(n, copy_n):
    """sbr_adam_step_zero_grad copies copy_n doubles src -> dst on its launch, no more, also when n < 256 (fewer elements than the
    copying workgroup has threads); the step itself is the one without a copy, bit for bit."""
    tensors = state(n, 5)
    src = torch.arange(1, 257, dtype=torch.float64, device=DEV) * 1.25
    dst = torch.full((GUARD + 256 + GUARD,), NAN, dtype=torch.float64, device=DEV)
    res = []
    for cn in (copy_n, 0):
        P, G, M, V = _bufs(tensors)
        view = dst[GUARD:]
        _launch(0, True, P, G, M, V, n, HYPERS[0], copy=(src.data_ptr() if cn else None, view.data_ptr() if cn else None, cn))
        res.append([b.check_untouched(None, 'copy')[0] for b in (P, G, M, V)])
    for a, b in zip(*res):
        _assert_bits(a, b, 'the step with a copy differs from the step without')
    host = dst.cpu()
    assert torch.equal(host[GUARD: GUARD + copy_n], src.cpu()[:copy_n])
    rest = torch.cat([host[:GUARD], host[GUARD + copy_n:]])
    assert bool(torch.isnan(rest).all()), 'more than copy_n doubles were written'


def test_argument_checks_and_the_empty_step():
    """Unknown kind, step = 0, copy_n = 257 and a copy with n = 0 are refused with a message in sbr_last_error; n = 0 returns OK and
    launches nothing: NaN-filled buffers (whose views are empty) stay NaN."""
    err = _L().SibrarHipError
    P, G, M, V = (_Buf(1, 4) for _ in range(4))               # four NaN each: a step over n = 0 of them
    src, dst = torch.ones(4, dtype=torch.float64, device=DEV), torch.full((4,), NAN, dtype=torch.float64, device=DEV)
    lr, wd, b1, b2, eps, _ = HYPERS[0]
    tail = (lr, b1, b2, eps, wd)
    for bad, match in [(lambda: call('sbr_adam_step', 2, P.ptr, G.ptr, M.ptr, V.ptr, 0, *tail, 1, stream()), 'unknown kind'),
                       (lambda: call('sbr_adam_step_zero_grad', -1, P.ptr, G.ptr, M.ptr, V.ptr, 0, *tail, 1, None, None, 0, stream()), 'unknown kind'),
                       (lambda: call('sbr_adam_step', 0, P.ptr, G.ptr, M.ptr, V.ptr, 0, *tail, 0, stream()), 'step must be >= 1'),
                       (lambda: call('sbr_adam_step_zero_grad', 0, P.ptr, G.ptr, M.ptr, V.ptr, 0, *tail, 0, None, None, 0, stream()), 'step must be >= 1'),
                       (lambda: call('sbr_adam_step_zero_grad', 0, P.ptr, G.ptr, M.ptr, V.ptr, 0, *tail, 1, src.data_ptr(), dst.data_ptr(), 257, stream()),
                        'bad copy request'),
                       (lambda: call('sbr_adam_step_zero_grad', 0, P.ptr, G.ptr, M.ptr, V.ptr, 0, *tail, 1, src.data_ptr(), dst.data_ptr(), 1, stream()),
                        'a copy needs a non-empty step')]:
        with pytest.raises(err, match=match):
            bad()
        assert match in _L().lib().sbr_last_error().decode()
    call('sbr_adam_step', 0, P.ptr, G.ptr, M.ptr, V.ptr, 0, *tail, 1, stream())
    call('sbr_adam_step_zero_grad', 1, P.ptr, G.ptr, M.ptr, V.ptr, 0, *tail, 1, None, None, 0, stream())
    call('sbr_adagrad_step', P.ptr, G.ptr, V.ptr, 0, 1e-2, 1e-10, 1e-2, stream())
    for b in (P, G, M, V):
        assert bool(torch.isnan(b.flat).all()), 'an empty step wrote something'
    assert bool(torch.isnan(dst).all()), 'a refused call copied'


# ---- FusedOptimizer branches ---------------------------------------------------------------------------------------------------
class _Two(torch.nn.Module):
    """two parameters of 35 and 7 elements: segments [0, 35) and [64, 71) of 128 flat elements, the rest padding"""

    def __init__(self):
        super().__init__()
        gen = torch.Generator().manual_seed(3)
        self.a = torch.nn.Parameter(torch.randn(5, 7, generator=gen))
        self.b = torch.nn.Parameter(torch.randn(7, generator=gen))


def _fused(name, wd=1e-2, seed=0):
    """-> (optimizer with a random state and gradient in its segments and zeros in its padding, mask of the segments)"""
    opt = S().FusedOptimizer(_Two().to(DEV), name, lr=1e-2, weight_decay=wd)
    fp = opt.fp
    assert fp.total == 128 and fp.offsets == [0, 64]
    seg = torch.zeros(128, dtype=torch.bool)
    seg[:35] = True
    seg[64:71] = True
    _, g, m, v = state(128, 40 + seed)
    for buf, src in ((fp.grad, g), (opt.m, v if name == 'adagrad' else m), (opt.v, v)):
        if buf is not None:
            buf.copy_(torch.where(seg, src, torch.zeros(128)).to(DEV))
    return opt, seg


def _snapshot(opt):
    return [t.cpu().clone() if t is not None else None for t in (opt.fp.flat, opt.fp.grad, opt.m, opt.v)]


@pytest.mark.parametrize('name', ['adamw', 'adam'])
@pytest.mark.parametrize('lo,hi', [(8, 40), (0, 64), (64, 128), (33, 70)])
def test_fused_optimizer_skip_leaves_the_range_alone(name, lo, hi):
    """step_flat(skip=(lo, hi)): [lo, hi) of flat, m and v bit-identical, every other element one step of the float64 rule (torch's
    defaults, which FusedOptimizer hard-codes) within the bound; with zero_grad and a copy the call returns True and exactly one of
    its launches carries the copy."""
    opt, _ = _fused(name)
    p, g, m, v = _snapshot(opt)
    src = torch.tensor([1.5, -2.0], dtype=torch.float64, device=DEV)
    dst = torch.zeros(2, dtype=torch.float64, device=DEV)
    lib = _L()
    lib.CALL_LOG = []
    try:
        assert opt.step_flat(skip=(lo, hi), zero_grad=True, copy=(src, dst)) is True
        torch.cuda.synchronize()
        log = lib.CALL_LOG
    finally:
        lib.CALL_LOG = None
    launches = [a for nm, a in log if nm == 'sbr_adam_step_zero_grad']
    assert len(launches) == (2 if lo > 0 and hi < 128 else 1) and sorted(a[14] for a in launches)[-1] == 2 and sum(a[14] for a in launches) == 2
    assert torch.equal(dst, src)
    p2, g2, m2, v2 = _snapshot(opt)
    inside = torch.zeros(128, dtype=torch.bool)
    inside[lo:hi] = True
    for a, b, nm in ((p2, p, 'flat'), (m2, m, 'm'), (v2, v, 'v'), (g2, g, 'grad')):
        _assert_bits(a[inside], b[inside], f'{nm}: the skipped range changed')
    assert not bool(_bits(g2[~inside]).any())
    refs, bounds = O.adam_ref(0 if name == 'adamw' else 1, p, g, m, v, 1e-2, 0.9, 0.999, 1e-8, 1e-2, 1)
    for o, r, b, nm in zip((p2, m2, v2), refs, bounds, 'pmv'):
        print(f'ratio {nm} {O.check_bound(o[~inside], r[~inside], b[~inside], f"skip {nm}"):.3f} skip')


def test_fused_optimizer_adagrad_with_zero_grad():
    """the adagrad branch: one step of the rule (eps 1e-10) within the bound, returns False, the gradient zeroed by its fill"""
    opt, _ = _fused('adagrad')
    p, g, s, _ = _snapshot(opt)
    assert opt.step_flat(zero_grad=True) is False
    p2, g2, s2, _ = _snapshot(opt)
    assert not bool(_bits(g2).any())
    refs, bounds = O.adagrad_ref(p, g, s, 1e-2, 1e-10, 1e-2)
    for o, r, b, nm in zip((p2, s2), refs, bounds, NAMES[2]):
        print(f'ratio {nm} {O.check_bound(o, r, b, f"fused adagrad {nm}"):.3f} fused adagrad')


@pytest.mark.parametrize('name', ['adamw', 'adam', 'adagrad'])
def test_fused_optimizer_padding_stays_zero(name):
    """the 64-element alignment padding between and behind the segments holds zeros in flat, m and v after four steps with weight decay"""
    opt, seg = _fused(name, wd=0.3)
    for t in range(4):
        opt.fp.grad.copy_(torch.where(seg, next_gradient(128, 9, t), torch.zeros(128)).to(DEV))
        opt.step_flat(zero_grad=t % 2 == 1)
    for t, nm in zip(_snapshot(opt), ('flat', 'grad', 'm', 'v')):
        if t is not None and nm != 'grad':
            assert bool((t[~seg] == 0).all()), f'{nm}: the padding moved'
            assert bool(torch.isfinite(t[seg]).all()) and bool((t[seg] != 0).any())


# ---- deferred row-wise kernels against the rule --------------------------------------------------------------------------------
R_ROWS, N_IDS, T_STEPS = 24, 30, 5
H_ROWS = (3e-3, 0.9, 0.999, 1e-8, 1e-2)              # lr, b1, b2, eps, wd


class _Table:
    """[R_ROWS, D] table behind one sentinel row of NaN: the pointer handed to the kernels is row 1, so a write to "row -1" (an id that
    the row map sends to -1) lands in the sentinel and is seen; _Buf's guards see the rest"""

    def __init__(self, D, data=None, fill=None):
        self.D = D
        self.buf = _Buf(R_ROWS + 1, D, fill=fill)
        self.buf.t[0] = NAN
        if data is not None:
            self.buf.t[1:] = data.to(DEV)
        self.ptr = self.buf.ptr + 4 * D

    def host(self, what):
        h = self.buf.check_untouched(None, what)
        assert bool(torch.isnan(h[0]).all()), f'{what}: the row in front of the table (row -1) was written'
        return h[1:].clone()


def _rows_world(D, seed, zero_state_rows):
    gen = torch.Generator().manual_seed(seed)
    p0, _, m0, v0 = (t.view(R_ROWS, D) for t in state(R_ROWS * D, seed))
    m0 = m0 * 1e-2
    v0 = (m0.double() ** 2 * _loguniform(R_ROWS * D, 0, 2, gen).view(R_ROWS, D) + 1e-12).float()      # |m| / sqrt(v) <= 1, as after real steps
    m0[zero_state_rows], v0[zero_state_rows] = 0.0, 0.0
    rowmap = torch.full((N_IDS,), -1, dtype=torch.int32)
    ids_with_row = torch.randperm(N_IDS, generator=gen)[:R_ROWS]
    rowmap[ids_with_row] = torch.randperm(R_ROWS, generator=gen).to(torch.int32)
    no_row = [i for i in range(N_IDS) if int(rowmap[i]) < 0]
    return gen, p0, m0, v0, rowmap, no_row


@pytest.mark.parametrize('kind', [0, 1])
@pytest.mark.parametrize('D', [1, 64, 65, 130])
@pytest.mark.parametrize('via', ['rows', 'step_rows'])
def test_deferred_rows_against_the_rule(kind, D, via):
    """sbr_adam_rows modes 0 / 1 / 2 and sbr_adam_step_rows (with a sweep of three sub-rows per step) on a 24-row table for five steps:
    id lists alternate between int32 and int64, go through a row map with -1 entries and repeat ids. After each step exactly the
    sub-rows of the named rows (and the swept ones) are current, every other row holds its old bits, and an id without a row writes
    nothing (the sentinel row in front of the table stays NaN). After the flush every row matches a float64 replay of the DENSE rule
    (zero gradient where the step named no row) within the sum of the propagated per-step bounds (optim_ref: e_in)."""
    lr, b1, b2, eps, wd = H_ROWS
    n_sub = (D + 63) // 64
    n_q = R_ROWS * n_sub
    gen, p0, m0, v0, rowmap, no_row = _rows_world(D, 11 * D + kind, zero_state_rows=slice(12, R_ROWS))
    P, M, V, G = _Table(D, p0), _Table(D, m0), _Table(D, v0), _Table(D, fill=0.0)
    rowmap_d = rowmap.to(DEV)
    claim, last = torch.zeros(n_q, dtype=torch.int32, device=DEV), torch.zeros(n_q, dtype=torch.int32, device=DEV)
    sched = torch.zeros(T_STEPS + 2, 2, device=DEV)
    hyper = (lr, b1, b2, eps, wd)
    ref, err = (p0.double(), m0.double(), v0.double()), None
    want_last = torch.zeros(n_q, dtype=torch.int32)
    rng = np.random.default_rng(D + kind)
    for t in range(1, T_STEPS + 1):
        ids = rng.integers(0, 12, size=6)                          # ids 12 .. 29 are never named: their rows replay everything at the flush
        ids[2] = ids[0]                                            # a duplicate
        ids[4] = no_row[t % len(no_row)]                           # an id without a row
        ids_d = _i64(ids) if t % 2 else _i32(ids)
        a64, a32 = (ids_d.data_ptr(), None) if t % 2 else (None, ids_d.data_ptr())
        rows = torch.unique(rowmap[torch.as_tensor(ids)].long())
        rows = rows[rows >= 0]
        before = [x.host(f'step {t}') for x in (P, M, V)]
        call('sbr_adam_rows', kind, 0, P.ptr, G.ptr, M.ptr, V.ptr, R_ROWS, D, a64, a32, rowmap_d.data_ptr(), len(ids), claim.data_ptr(),
             last.data_ptr(), sched.data_ptr(), *hyper, t, stream())
        grad = torch.zeros(R_ROWS, D)
        grad[rows] = next_gradient(R_ROWS * D, D, t).view(R_ROWS, D)[rows]
        G.buf.t[1:] = grad.to(DEV)
        swept = torch.zeros(n_q, dtype=torch.bool)
        if via == 'rows':
            call('sbr_adam_rows', kind, 1, P.ptr, G.ptr, M.ptr, V.ptr, R_ROWS, D, a64, a32, rowmap_d.data_ptr(), len(ids), claim.data_ptr(),
                 last.data_ptr(), sched.data_ptr(), *hyper, t, stream())
        else:
            sweep_lo = (3 * (t - 1) + 20 * n_sub) % n_q                # starts among the never-named rows, wraps around the table's end
            swept[(sweep_lo + torch.arange(3)) % n_q] = True
            call('sbr_adam_step_rows', kind, P.ptr, G.ptr, M.ptr, V.ptr, R_ROWS * D, 0, R_ROWS * D, D, a64, a32, rowmap_d.data_ptr(), len(ids),
                 claim.data_ptr(), last.data_ptr(), sched.data_ptr(), *hyper, t, sweep_lo, 3, None, None, 0, stream())
        assert not bool(_bits(G.host(f'gradient after step {t}')).any()), 'the consumed gradient rows were not zeroed'
        named = torch.zeros(R_ROWS, dtype=torch.bool)
        named[rows] = True
        named_q = named.repeat_interleave(n_sub)
        want_last[named_q | swept] = t
        assert torch.equal(last.cpu(), want_last), f'step {t}: other sub-rows than the named (and swept) ones were brought up to date'
        idle = (~(named_q | swept)).view(R_ROWS, n_sub).repeat_interleave(64, dim=1)[:, :D]
        for x, b, nm in zip((P, M, V), before, 'pmv'):
            _assert_bits(x.host(f'{nm} after step {t}')[idle], b[idle], f'{nm}: a sub-row that step {t} neither named nor swept changed')
        ref, err = O.adam_ref(kind, ref[0], grad, ref[1], ref[2], lr, b1, b2, eps, wd, t, e_in=err)
    call('sbr_adam_rows', kind, 2, P.ptr, None, M.ptr, V.ptr, R_ROWS, D, None, None, None, 0, None, last.data_ptr(), sched.data_ptr(), *hyper,
         T_STEPS, stream())
    assert bool((last.cpu() == T_STEPS).all())
    for x, r, b, nm in zip((P, M, V), ref, err, 'pmv'):
        print(f'ratio {nm} {O.check_bound(x.host("flush"), r, b, f"deferred {via} D {D} {nm}"):.3f} deferred {via} kind {kind} D {D}')


def test_deferred_adamw_with_eps_zero_equals_the_dense_kernel_and_torch():
    """eps = 0, AdamW, rows that never receive a gradient (m = v = 0): the dense step divides 0 by sqrt(0) / sqrt(bc2) + 0 and the
    parameter becomes NaN, as in torch.optim.AdamW. The deferred replay must not take its idle short cut there (adam_wave_is_idle
    requires eps > 0): after three steps and a flush the table equals the dense kernel's — NaN where it has NaN, the same bits
    elsewhere — and torch.optim.AdamW in float64 has NaN in exactly the same rows."""
    D, T = 80, 3
    n_sub = 2
    lr, b1, b2, wd = 3e-3, 0.9, 0.999, 1e-2
    gen = torch.Generator().manual_seed(17)
    p0 = torch.randn(R_ROWS, D, generator=gen) * 0.1
    grads = [torch.zeros(R_ROWS, D) for _ in range(T)]
    for t in range(T):
        grads[t][t: t + 4] = torch.randn(4, D, generator=gen)     # rows 0 .. 3 from the first step on, rows 4 and 5 later, rows 6 .. 23 never
    # dense kernel
    Pd, Gd, Md, Vd = _bufs([p0.reshape(-1), torch.zeros(R_ROWS * D), torch.zeros(R_ROWS * D), torch.zeros(R_ROWS * D)])
    # deferred
    P, M, V, G = _Table(D, p0), _Table(D, fill=0.0), _Table(D, fill=0.0), _Table(D, fill=0.0)
    claim, last = torch.zeros(R_ROWS * n_sub, dtype=torch.int32, device=DEV), torch.zeros(R_ROWS * n_sub, dtype=torch.int32, device=DEV)
    sched = torch.zeros(T + 2, 2, device=DEV)
    # torch
    pt = torch.nn.Parameter(p0.double().clone())
    topt = torch.optim.AdamW([pt], lr=lr, betas=(b1, b2), eps=0.0, weight_decay=wd)
    for t in range(1, T + 1):
        Gd.t.copy_(grads[t - 1].view(1, -1).to(DEV))
        call('sbr_adam_step', 0, Pd.ptr, Gd.ptr, Md.ptr, Vd.ptr, R_ROWS * D, lr, b1, b2, 0.0, wd, t, stream())
        ids = _i32(np.arange(t - 1, t + 3))
        for mode in (0, 1):
            if mode == 1:
                G.buf.t[1:] = grads[t - 1].to(DEV)
            call('sbr_adam_rows', 0, mode, P.ptr, G.ptr, M.ptr, V.ptr, R_ROWS, D, None, ids.data_ptr(), None, 4, claim.data_ptr(), last.data_ptr(),
                 sched.data_ptr(), lr, b1, b2, 0.0, wd, t, stream())
        pt.grad = grads[t - 1].double()
        topt.step()
    call('sbr_adam_rows', 0, 2, P.ptr, None, M.ptr, V.ptr, R_ROWS, D, None, None, None, 0, None, last.data_ptr(), sched.data_ptr(), lr, b1, b2, 0.0, wd,
         T, stream())
    dense = [b.check_untouched(None, 'dense')[0].view(R_ROWS, D) for b in (Pd, Md, Vd)]
    idle_once = torch.zeros(R_ROWS, dtype=torch.bool)          # rows that took a step with m = v = g = 0: all but the first four
    idle_once[4:] = True
    assert bool(torch.isnan(dense[0][idle_once]).all()) and bool(torch.isfinite(dense[0][~idle_once]).all())
    assert torch.equal(torch.isnan(pt.detach()), torch.isnan(dense[0])), 'the dense kernel and torch.optim.AdamW disagree about the NaN rows'
    for x, d, nm in zip((P, M, V), dense, 'pmv'):
        got = x.host(f'eps = 0 {nm}')
        nan = torch.isnan(d)
        assert torch.equal(torch.isnan(got), nan), f'{nm}: the deferred path and the dense kernel disagree about NaN ({int(nan.sum())} in the dense result, {int(torch.isnan(got).sum())} here)'
        _assert_bits(got[~nan], d[~nan], f'{nm}: eps = 0')
