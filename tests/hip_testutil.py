"""Helpers shared by the kernel-level GPU tests (tests/test_hip_rowops.py, tests/test_hip_tail.py): the ctypes call wrapper, operands as
strided / shifted views inside NaN-filled buffers with the "nothing outside the addressed rows was written" check, and the bound
assertions. u = 2^-24 is the unit roundoff of fp32; see the header of test_hip_rowops.py for the conventions. A plain module: no
fixtures, no pytest hooks."""
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
