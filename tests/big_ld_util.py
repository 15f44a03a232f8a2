"""What the sibling modules of tests/test_hip_big_ld.py share (tests/test_hip_big_ld_gemm.py, tests/test_hip_big_ld_rows.py): the three
operand layouts (a _BigLd view at LD_BIG, the same operand at ld = 192 — 256 or 320 where a row is wider —, and compact), the run-in-both-
layouts comparison, the guard-band checks, and the index vectors that send traffic to the rows on each side of both wraps. A plain
module: no fixtures, no pytest hooks."""
import numpy as np
import torch

from hip_testutil import DEV, _BigLd, _Buf, _assert_bits, _bits

LD_SMALL = 192
N = 130                                      # rows of a view that crosses element 2^31 (row 64) and element 2^32 (row 128)
EDGE_ROWS = (0, 63, 64, 65, 127, 128, 129)   # the first row, and the rows on each side of both wraps


def _t(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))


def big(rows, cols, data=None, fill=None):
    return _BigLd(rows, cols, data=None if data is None else _t(data), fill=fill)


class _Kept(_Buf):
    """a _Buf that remembers the view as it was handed out, as _BigLd does: a prefilled table's rows that no index names are compared
    with that bit for bit (the whole-buffer NaN check of _Buf still covers everything outside the view)"""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.before = _bits(self.t.contiguous().cpu())

    def check_untouched(self, written_rows=None, what=''):
        host = super().check_untouched(None, what)
        may = torch.zeros(self.rows, dtype=torch.bool)
        may[slice(None) if written_rows is None else written_rows] = True
        same = _bits(host.contiguous())[~may] == self.before[~may]
        assert bool(same.all()), f'{what}: {int((~same).sum())} elements of rows outside the addressed ones were written'
        return host


def small(rows, cols, data=None, fill=None):
    """ld = 192, a multiple of 64 like LD_BIG; 256 or 320 where a row is wider"""
    return _Kept(rows, cols, ld=LD_SMALL if cols <= LD_SMALL else (256 if cols <= 256 else 320), data=None if data is None else _t(data), fill=fill)


def compact(rows, cols, data=None, fill=None):
    return _Kept(rows, cols, data=None if data is None else _t(data), fill=fill)


BOTH = ((big, 'ld = LD_BIG'), (small, 'ld = 192'))


def unchanged(buf, data, what):
    """an input: what surrounds the view holds its NaN pattern, and the view holds the bits it was given"""
    _assert_bits(buf.check_untouched(what=what).contiguous(), _t(data).reshape(buf.rows, buf.cols).float(), f'{what} was written')


def out(buf, rows=None, what=''):
    """the view on the host after the guard check; ``rows``: the rows the call may write (None: all), every other row keeps its bits"""
    if rows is not None:
        m = torch.zeros(buf.rows, dtype=torch.bool)
        m[torch.as_tensor(np.asarray(rows), dtype=torch.long)] = True
        rows = m
    return buf.check_untouched(rows, what=what).contiguous()


def both(run, what):
    """run(make) -> a tensor or a tuple of tensors, once per layout; the LD_BIG result, after checking that the two agree in bits"""
    got = [run(make) for make, _ in BOTH]
    for a, b in zip(*[g if isinstance(g, tuple) else (g,) for g in got]):
        a, b = (v if v.dtype == torch.float32 else v.to(torch.int32).view(torch.float32) for v in (a, b))
        _assert_bits(a, b, f'{what}: {BOTH[0][1]} against {BOTH[1][1]}')
    return got[0]


def covers(idx, what):
    """the index vector names every row of EDGE_ROWS (asserted before the kernel is called)"""
    missing = sorted(set(EDGE_ROWS) - set(int(v) for v in np.asarray(idx).reshape(-1)))
    assert not missing, f'{what} sends nothing to rows {missing}'
    return idx


def perm_rows(seed, n=N):
    """a permutation of the n rows"""
    return covers(np.random.default_rng(seed).permutation(n).astype(np.int64), 'the permutation')


def draw_rows(count, seed, n=N):
    """``count`` draws with repeats from the n rows; the rows of EDGE_ROWS are among them at random positions"""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, n, size=count).astype(np.int64)
    r[rng.permutation(count)[:len(EDGE_ROWS)]] = EDGE_ROWS
    return covers(r, 'the draw')


def some_rows(count, seed, n=N):
    """``count`` < n distinct rows, the rows of EDGE_ROWS among them: the other n - count rows of the table are named by nothing"""
    rng = np.random.default_rng(seed)
    rest = np.setdiff1d(np.arange(n), EDGE_ROWS)
    r = np.concatenate([np.asarray(EDGE_ROWS), rng.permutation(rest)[:count - len(EDGE_ROWS)]])
    return covers(rng.permutation(r).astype(np.int64), 'the injective map')


def ws(nbytes):
    return torch.empty(max(nbytes // 4, 1), device=DEV)
