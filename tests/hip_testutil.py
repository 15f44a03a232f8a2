"""Helpers shared by the kernel-level GPU tests (tests/test_hip_rowops.py, tests/test_hip_tail.py): the ctypes call wrapper, operands as
strided / shifted views inside NaN-filled buffers with the "nothing outside the addressed rows was written" check, and the bound
assertions. u = 2^-24 is the unit roundoff of fp32; see the header of test_hip_rowops.py for the conventions. A plain module: no
fixtures, no pytest hooks. ``_BigLd`` (for tests/test_hip_big_ld.py) is the same kind of view at a leading dimension of 2^25 + 64
elements inside one untouched 16.1 GiB buffer, with guard bands in place of the whole-buffer check."""
import importlib

import numpy as np
import torch

DEV = 'cuda'
U32 = 2.0 ** -24
NAN = float('nan')
GUARD = 64                                   # guard elements in front of and behind a view (a multiple of 4: keeps the alignment)
INT_GUARD = {torch.int32: -0x5A5A5A5B, torch.uint8: 0xA5}            # what an integer _Buf holds where a float one holds NaN
EXP_ULP = 4 * U32                            # allowed relative error of one expf / logf / tanhf call (2 ulp)
SELU_A, SELU_S = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946
SELU_AF, SELU_SF = float(np.float32(SELU_A)), float(np.float32(SELU_S))
LIP = {0: 1.0, 1: 1.0, 2: 1.0, 3: 0.25, 4: SELU_SF * SELU_AF}        # Lipschitz constants of the activations


def ref_act(pre, act):
    """the activation codes of include/sibrar_hip.h in the dtype of ``pre``, with the fp32 selu constants of the kernels"""
    if act == 1:
        return torch.relu(pre)
    if act == 2:
        return torch.tanh(pre)
    if act == 3:
        return torch.sigmoid(pre)
    if act == 4:
        return SELU_SF * torch.where(pre > 0, pre, SELU_AF * torch.expm1(pre))
    return pre


def ref_act_grad_from_out(y, act):
    """d act / d pre-activation through the activation's OUTPUT (float64), with the fp32 selu constants of the kernels"""
    if act == 1:
        return (y > 0).double()
    if act == 2:
        return 1 - y * y
    if act == 3:
        return y * (1 - y)
    if act == 4:
        return torch.where(y > 0, torch.full_like(y, SELU_SF), y + SELU_SF * SELU_AF)
    return torch.ones_like(y)


def act_grad_err(y, act):
    """bound of the fp32 evaluation of act'(y) on an fp32 y: relu / selu(y > 0) / none exact; 1 - y y: two roundings, each relative to
    at most max(y^2, |1 - y^2|) <= y^2 + |g|; y (1 - y): two roundings relative to |g|; y + c: one rounding, and c = scale * alpha is
    itself the fp32 product of the two fp32 constants (u c)"""
    g = ref_act_grad_from_out(y, act).abs()
    if act == 2:
        return 2 * U32 * (g + y * y)
    if act == 3:
        return 2 * U32 * g
    if act == 4:
        return torch.where(y > 0, torch.zeros_like(g), U32 * (g + SELU_SF * SELU_AF))
    return torch.zeros_like(g)


def S():
    import sibrar_amd
    return sibrar_amd


def _L():
    return importlib.import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')


def call(name, *args):
    _L().call(name, *args)
    torch.cuda.synchronize()


def stream():
    return _L().stream()


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _dev(t):
    return None if t is None else t.to(DEV)


def _p(t):
    return None if t is None else t.data_ptr()


class _Buf:
    """A [rows, cols] fp32 view with row stride ld >= cols inside a NaN-filled flat buffer; ``off`` elements (4 bytes each) shift the
    base pointer off the allocation's 16-byte boundary. An integer ``dtype`` (int32, uint8) is filled with its INT_GUARD pattern."""

    def __init__(self, rows, cols, ld=None, off=0, data=None, fill=None, dtype=torch.float32):
        self.rows, self.cols, self.ld, self.off = rows, cols, ld or cols, off
        assert self.ld >= cols
        self.guard = NAN if dtype.is_floating_point else INT_GUARD[dtype]
        self.flat = torch.full((GUARD + off + rows * self.ld + GUARD,), self.guard, device=DEV, dtype=dtype)
        self.t = self._view(self.flat)
        assert (self.t.data_ptr() - self.flat.data_ptr()) == (GUARD + off) * self.flat.element_size()
        if data is not None:
            self.t.copy_(data.to(DEV))
        elif fill is not None:
            self.t.fill_(fill)

    def _view(self, flat):
        return flat[GUARD + self.off: GUARD + self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]

    @property
    def ptr(self):
        return self.t.data_ptr()

    def host(self):
        return self.t.cpu()

    def check_untouched(self, written_rows=None, what=''):
        """every element outside [written_rows, :cols] still holds the NaN pattern; -> the view on the host"""
        host = self.flat.cpu()
        may = torch.zeros(host.shape, dtype=torch.bool)
        mv = self._view(may)
        if written_rows is None:
            mv[:] = True
        else:
            mv[written_rows] = True
        kept = torch.isnan(host[~may]) if host.dtype.is_floating_point else host[~may] == self.guard
        assert bool(kept.all()), f'{what}: {int((~kept).sum())} elements outside the addressed rows / columns were written'
        return self._view(host)


LD_BIG = (1 << 25) + 64                     # a leading dimension that puts row 64 past element 2^31 and row 128 past element 2^32
BIG_ROWS = 130                               # the most rows a _BigLd view may have
BIG_ELEMS = (BIG_ROWS - 1) * LD_BIG + 1024   # fp32 elements of the one buffer (about 16.1 GiB); the last row may be up to 960 wide
BIG_HEADROOM = 4 << 30                       # free device memory asked for beyond the buffer
NAN_BITS = 0x7FC00000                        # what torch writes for float('nan'): the fill pattern of _Buf, compared bit for bit
_BIG = {'flat': None}


def big_ld_crossings(rows):
    """which wraps a view of ``rows`` rows at LD_BIG can show: the start of its last row lies past element 2^31 (an int product wraps
    negative), past element 2^32 (an unsigned product wraps), past byte 2^32 (a 32-bit byte offset wraps)"""
    last = (rows - 1) * LD_BIG
    return {'2^31 elements': last >= 1 << 31, '2^32 elements': last >= 1 << 32, '2^32 bytes': 4 * last >= 1 << 32}


class _BigLd:
    """A [rows, cols] fp32 view with row stride LD_BIG into ONE lazily allocated, never filled buffer of BIG_ELEMS elements (module
    level: a second _BigLd reuses it, so only one is in use at a time; ``release()`` frees it). rows <= 130: row 64 starts past
    element 2^31, row 128 past element 2^32, every row from 32 on past byte 2^32. In place of _Buf's whole-buffer check there is a
    guard band: the GUARD elements behind each row's ``cols`` and in front of each row start except row 0 (the view starts at the
    buffer's first element) hold the NaN pattern and are compared bit for bit afterwards (the last row's band ends where the buffer
    ends); the view itself is remembered as it was handed out, and rows the call must not write are compared with that bit for bit."""

    def __init__(self, rows, cols, ld=None, off=0, data=None, fill=None):
        assert ld in (None, LD_BIG) and off == 0 and 1 <= rows <= BIG_ROWS and 1 <= cols <= LD_BIG - 2 * GUARD
        self.rows, self.cols, self.ld = rows, cols, LD_BIG
        self.crossings = big_ld_crossings(rows)
        if rows > 128:
            assert all(self.crossings.values()), self.crossings
        flat = self._flat()
        self.t = flat.as_strided((rows, cols), (LD_BIG, 1))
        tail = min(GUARD, BIG_ELEMS - ((rows - 1) * LD_BIG + cols))
        assert tail > 0
        self.bands = [flat.as_strided((rows - 1, GUARD), (LD_BIG, 1), cols), flat.as_strided((1, tail), (LD_BIG, 1), (rows - 1) * LD_BIG + cols)]
        if rows > 1:
            self.bands.append(flat.as_strided((rows - 1, GUARD), (LD_BIG, 1), LD_BIG - GUARD))
        for b in self.bands:
            b.fill_(NAN)
        if data is not None:
            self.t.copy_(data.to(DEV))
        else:
            self.t.fill_(NAN if fill is None else fill)
        self.before = _bits(self.t.contiguous().cpu())
        assert self.t.data_ptr() == flat.data_ptr() and self.t[rows - 1].data_ptr() - flat.data_ptr() == 4 * (rows - 1) * LD_BIG

    @staticmethod
    def _flat():
        if _BIG['flat'] is None:
            import pytest
            free, _ = torch.cuda.mem_get_info()
            if free < 4 * BIG_ELEMS + BIG_HEADROOM:
                pytest.skip(f'{free} bytes of device memory free, {4 * BIG_ELEMS + BIG_HEADROOM} needed (the buffer and 4 GiB)')
            _BIG['flat'] = torch.empty(BIG_ELEMS, device=DEV, dtype=torch.float32)
        return _BIG['flat']

    @staticmethod
    def release():
        _BIG['flat'] = None
        torch.cuda.empty_cache()

    @property
    def ptr(self):
        return self.t.data_ptr()

    def host(self):
        return self.t.contiguous().cpu()

    def check_untouched(self, written_rows=None, what=''):
        """the guard bands still hold the NaN pattern and every row outside ``written_rows`` (None: every row may be written) holds
        the bits it was handed out with; -> the view on the host"""
        for b in self.bands:
            kept = _bits(b.contiguous().cpu()) == NAN_BITS
            assert bool(kept.all()), f'{what}: {int((~kept).sum())} guard elements around the rows were written'
        host = self.host()
        may = torch.zeros(self.rows, dtype=torch.bool)
        may[slice(None) if written_rows is None else written_rows] = True
        same = _bits(host)[~may] == self.before[~may]
        assert bool(same.all()), f'{what}: {int((~same).sum())} elements of rows outside the addressed ones were written'
        return host


def _i32(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.int32).to(DEV)


def _i64(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.int64).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_bits(got, ref, what=''):
    assert got.shape == ref.shape, what
    bad = _bits(got) != _bits(ref)
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} of {bad.numel()} elements differ in bits'


def _assert_bound(got, ref, bound, what=''):
    """|got - ref| <= bound elementwise (float64); NaN anywhere fails"""
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    assert not bool(bad.any()), (f'{what}: {int(bad.sum())} of {bad.numel()} elements over the bound, worst err {float(err[bad].max()):.3e} '
                                 f'at bound {float(bound[bad][err[bad].argmax()]):.3e}')


def _ulp(x):
    """spacing of fp32 at |x| (float64 tensor)"""
    x = x.abs().double().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(x)) - 23)


def _orders(n, n_table, seed, hot=None):
    """index lists with heavy duplication in random, sorted and reversed order; ``hot``: one row named by > 1,000 sources (if n allows)"""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, n_table, size=n)
    if hot is not None and n >= 1500:
        r[rng.choice(n, size=1200, replace=False)] = hot
    return {'random': r, 'sorted': np.sort(r), 'reversed': np.sort(r)[::-1].copy()}
