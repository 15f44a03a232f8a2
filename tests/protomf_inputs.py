"""Inputs for the ProtoMF kernel tests whose arg-mins cannot flip between fp32 and float64 — a test helper, not a test.

The regularisers of ProtoMF route a gradient through ``min`` over the prototypes of a row and ``min`` over the rows of a prototype. When
the best and the runner-up of such a minimum are closer than the rounding error, fp32 and float64 pick different entries and the
gradient changes discretely: that is a property of the function, not an error of either implementation. So the inputs are constructed:
after drawing, every row whose float64 best / runner-up margin is below MARGIN is redrawn (fixed seed, on the CPU), and for every
prototype column with such a margin the winning row is redrawn, until none remain.

MARGIN = 1e-4 is three orders of magnitude above the fp32 error of a similarity (a few 2^-24 on values in [0, 2]).

D = 1 is the one shape where this cannot be done: a cosine of one-element vectors is exactly +-1, every similarity is exactly 0 or 2 in
every precision, and minima tie exactly. There the margins are exactly 0 or 2 (``exact_only``), the ties are exact in fp32 and float64
alike, and the gradient of x / |x| is identically zero, so which of the tied entries receives the regulariser's gradient has no effect.
"""
import torch
from torch.nn import functional as F

MARGIN = 1e-4


def margins(e64, p64):
    """float64 best / runner-up margins of the distances 2 - sim: per row (over the prototypes) and per prototype (over the rows)."""
    dis = 2 - torch.clamp(1 + F.normalize(e64) @ F.normalize(p64).T, min=0., max=2.)
    r2 = torch.topk(dis, 2, dim=1, largest=False).values
    c2 = torch.topk(dis, 2, dim=0, largest=False).values if dis.shape[0] > 1 else None
    col = c2[1] - c2[0] if c2 is not None else torch.full((dis.shape[1],), 2.0, dtype=dis.dtype)
    return r2[:, 1] - r2[:, 0], col


def make_safe(table, used, protos, gen, scale):
    """Redraw rows of ``table`` (in place; ``used``: the distinct table rows a batch names) until every margin is >= MARGIN."""
    if table.shape[1] == 1:
        return 0
    used = torch.as_tensor(used).long()
    redrawn = 0
    for _ in range(200):
        e = table[used].double()
        row_m, col_m = margins(e, protos.double())
        dis = 2 - torch.clamp(1 + F.normalize(e) @ F.normalize(protos.double()).T, min=0., max=2.)
        bad = torch.zeros(len(used), dtype=torch.bool)
        bad[row_m < MARGIN] = True
        bad[dis.argmin(dim=0)[col_m < MARGIN]] = True
        n = int(bad.sum())
        if n == 0:
            return redrawn
        table[used[bad]] = (torch.randn(n, table.shape[1], generator=gen) * scale).to(table.dtype)
        redrawn += n
    raise AssertionError('the redraws did not converge')


def argmin_safe(R, D, P, seed, scale=0.5):
    """-> (table [R, D] fp32, rows int32 [R] — a permutation, so the lookup is exercised and no row repeats —, prototypes [P, D] fp32)"""
    gen = torch.Generator().manual_seed(seed)
    table = torch.randn(R, D, generator=gen) * scale
    protos = torch.randn(P, D, generator=gen)
    rows = torch.randperm(R, generator=gen).to(torch.int32)
    make_safe(table, torch.arange(R), protos, gen, scale)
    return table, rows, protos


def exact_only(m):
    """D = 1: every margin is exactly 0 or exactly 2"""
    return bool(((m == 0) | (m == 2)).all())
