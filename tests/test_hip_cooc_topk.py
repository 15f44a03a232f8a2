"""'sbr_cooc_weight_topk' (csrc/ultragcn.hip, ``ops.cooc_weight_topk``) on the GPU: bit for bit against the numpy float32 restatement of
tests/ultragcn_ref.py — ties are canonical, so every position of every list is compared — over three matrices, k = 1 / 10 / 64, both
settings of include_self, a split of the rows, several tiles, an all-zero column, an item with fewer candidates than k and repeated runs;
the float32 values against float64 within 2 u; ``ops.ultragcn_scales`` against the float64 scales."""
import functools

import numpy as np
import pytest
import torch

import ultragcn_ref as R
from hip_testutil import DEV, S

pytestmark = pytest.mark.gpu
SHAPES = {(65, 33): 0.2, (130, 257): 0.06, (300, 1100): 0.02}


@functools.lru_cache(maxsize=None)
def world(shape):
    """(matrix, resident matrix, float32 scales on host and device, the restatement's value matrix and counts): computed once per shape"""
    Sm = S()
    x = R.matrix(*shape, SHAPES[shape], seed=3, empty_items=(3,))
    features = __import__('importlib').import_module(Sm.ops.__name__.rsplit('.', 1)[0] + '.features')
    csr = features.DeviceCSR(x).to(DEV)
    _, _, row, col = R.scales32(x)
    v, G = R.values32(x, row, col)
    assert R.has_value_tie(v, G), 'no exact tie in the case: the index rule would go unchecked'
    return x, csr, (row, col), (torch.from_numpy(row).to(DEV), torch.from_numpy(col).to(DEV)), v, G


def run(shape, k, include_self=True, **kw):
    _, csr, _, (row, col), _, _ = world(shape)
    idx, val, length = S().ops.cooc_weight_topk(csr, row, col, k, include_self=include_self, **kw)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy(), length.cpu().numpy()


def same(got, want, what):
    for g, w, name in zip(got, want, ('idx', 'val', 'len')):
        assert g.dtype == w.dtype and g.shape == w.shape, f'{what}: {name} {g.dtype} {g.shape}'
        bad = g.view(np.int32) != w.view(np.int32)
        assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.size} positions of {name} differ in bits'


@pytest.mark.parametrize('k,include_self', [(1, True), (10, True), (10, False), (64, True), (64, False)])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_lists_equal_the_float32_restatement_bit_for_bit(shape, k, include_self):
    x, _, _, _, v, G = world(shape)
    want = R.select(v, G, k, include_self)
    got = run(shape, k, include_self)
    same(got, want, f'{shape} k={k} self={include_self}')
    m = shape[1]
    assert got[2][3] == 0 and np.all(got[0][3] == -1), 'the all-zero column has an empty list'
    assert got[2][m - 1] == min(k, 2 if include_self else 1), 'the lonely pair has two candidates, itself among them'
    if k > 2:
        assert got[2][m - 1] < k and got[0][m - 1, -1] == -1 and got[1][m - 1, -1] == 0
    if include_self and k == 64:
        assert all(i in got[0][i, :got[2][i]] for i in range(m) if 0 < got[2][i] < k), 'a short list holds its own item'
    same(run(shape, k, include_self), got, 'a second run')


@pytest.mark.parametrize('shape', list(SHAPES))
def test_a_split_of_the_rows_and_of_the_columns_equals_the_whole(shape):
    m = shape[1]
    whole = run(shape, 10)
    cut = m // 3
    a, b = run(shape, 10, rows=(0, cut)), run(shape, 10, rows=(cut, m))
    assert np.all(a[2][cut:] == 0) and np.all(a[0][cut:] == -1) and np.all(b[2][:cut] == 0), 'rows outside the range come back empty'
    merged = tuple(np.concatenate([p[:cut], q[cut:]]) for p, q in zip(a, b))
    same(merged, whole, 'rows split')
    same(run(shape, 10, tile_cols=64), whole, 'tiles of 64 columns')
    same(run(shape, 64, tile_cols=64), run(shape, 64), 'tiles of 64 columns, k = 64')


def test_values_are_within_2u_of_float64_and_refusals():
    Sm = S()
    shape = (130, 257)
    x, csr, (row, col), (rowd, cold), v, G = world(shape)
    idx, val, length = run(shape, 64)
    om, _ = R.omega64(x, row, col)
    worst = 0.
    for i in range(shape[1]):
        j = idx[i, :length[i]]
        rel = np.abs(val[i, :length[i]].astype(np.float64) - om[i, j]) / om[i, j]
        worst = max(worst, float(rel.max(initial=0.)))
    print(f'largest relative error of a list value against float64: {worst / R.U:.3f} u (allowed {float(R.gamma(2)) / R.U:.3f} u)')
    assert worst <= R.gamma(2)
    for k in (0, 65):
        with pytest.raises(Sm.SibrarHipError, match='sbr_cooc_weight_topk: k='):
            Sm.ops.cooc_weight_topk(csr, rowd, cold, k)
    with pytest.raises(ValueError, match='row_scale'):
        Sm.ops.cooc_weight_topk(csr, rowd[:-1], cold, 5)


@pytest.mark.parametrize('shape', list(SHAPES))
def test_the_scale_vectors_on_the_device(shape):
    x, csr, _, _, _, _ = world(shape)
    got = [t.cpu().numpy() for t in S().ops.ultragcn_scales(csr)]
    want64 = R.scales64(x)
    for g, w, name in zip(got, want64, ('beta_u', 'beta_i', 'row_scale', 'col_scale')):
        assert g.dtype == np.float32 and g.shape == w.shape
        assert np.all(np.abs(g.astype(np.float64) - w) <= R.U * np.abs(w)), f'{name}: not the float64 value rounded to float32 once'
        assert np.array_equal(g == 0, w == 0), f'{name}: the zeros (no interactions) differ'
