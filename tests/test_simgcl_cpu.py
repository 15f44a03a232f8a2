"""The references of the noisy propagation (tests/simgcl_ref.py) checked against each other and against tests/naive_ref.py, and the
host side of simgcl.py: the generator's counter layout, the fp32 restatement against float64 inside its own bound, the length of a row's
noise, the Horner form of the backward pass against float64 autograd, the constructors and the registry. No GPU."""
import numpy as np
import pytest
import torch

import lightgcn_ref as L
import naive_ref as N
import simgcl_ref as R


def test_noise_ref_is_the_generator_of_naive_ref_on_the_matching_counter():
    """The counter here is (row, column / 4, stream low, stream high); uniform_rows_ref's is (id low, id high, item / 4, 0). So: the
    known-answer vectors of naive_ref read in this layout, and uniform_rows_ref where the two layouts meet: block 0 of stream_id = 0
    against user id = row, item block 0."""
    for key, counter, answer in N.KNOWN_ANSWERS:
        seed = key[0] | (key[1] << 32)
        row, block, stream = counter[0], counter[1], counter[2] | (counter[3] << 32)
        got = R.noise_ref(seed, stream, [row], 4 * block + 4)[0, 4 * block:]
        assert np.array_equal(got, N.unit_float(np.array(answer, dtype=np.uint32))), (key, counter)
    rows = np.array([0, 1, 7, 2 ** 24 - 1])
    for seed in (0, 3, 0x123456789ABCDEF0):
        assert np.array_equal(R.noise_ref(seed, 0, rows, 4), N.uniform_rows_ref(seed, rows, 4))
        assert np.array_equal(R.noise_ref(seed, 0, rows, 3), N.uniform_rows_ref(seed, rows, 3))
    a, b = R.noise_ref(5, R.stream_id(2, 1, 3), np.arange(6), 13), R.noise_ref(5, R.stream_id(2, 1, 3), np.arange(3, 6), 13)
    assert np.array_equal(a[3:], b), 'a value depends on the row id, not on its place'
    assert a.dtype == np.float32 and bool((a >= 0).all()) and bool((a < 1).all())
    others = [R.noise_ref(6, R.stream_id(2, 1, 3), np.arange(6), 13), R.noise_ref(5, R.stream_id(2, 1, 2), np.arange(6), 13),
              R.noise_ref(5, R.stream_id(2, 2, 3), np.arange(6), 13), R.noise_ref(5, R.stream_id(3, 1, 3), np.arange(6), 13),
              R.noise_ref(5, 1 << 32, np.arange(6), 13)]
    assert all(not np.array_equal(a, o) for o in others)
    ids = {R.stream_id(s, v, k) for s in range(3) for v in range(4) for k in range(64)}
    assert len(ids) == 3 * 4 * 64


@pytest.mark.parametrize('d', [1, 3, 4, 5, 63, 64, 65, 128, 260, 512])
def test_the_summation_order_against_float64(d):
    nb, g4 = R.group_of(d)
    assert g4 >= min(nb, 64) and g4 & (g4 - 1) == 0 and (g4 == 1 or g4 // 2 < nb)
    u = R.noise_ref(1, 9, np.arange(50), d)
    q = R.sumsq32(u)
    q64 = (u.astype(np.float64) ** 2).sum(1)
    k = 4 * -(-nb // g4) + int(np.log2(g4)) + 1
    assert k <= 15
    assert bool((np.abs(q.astype(np.float64) - q64) <= L.gamma(k) * q64).all())
    if d <= 4:                                                               # one partial sum: plain left-to-right fp32
        want = np.zeros(50, dtype=np.float32)
        for c in range(d):
            want = want + u[:, c] * u[:, c]
        assert np.array_equal(q, want)


@pytest.mark.parametrize('d', [1, 5, 64, 260])
@pytest.mark.parametrize('shape', [(5, 64), (257, 3)])
def test_restatement_against_float64_within_its_bound(shape, d):
    g = L.world(*shape)
    x, s0 = L.table(g.n, d, 1), L.table(g.n, d, 2)
    eps, seed, stream, scale = 0.1, 11, R.stream_id(4, 1, 2), 1.0 / 3
    y, s = R.propagate_noise32(g, x, eps, seed, stream, s0, scale)
    y64 = R.propagate_noise64(g, x, eps, seed, stream)
    by, bs, near, slack = R.propagate_noise_bound(g, x, eps, seed, stream, s0, scale)
    assert near.mean() <= 0.01
    assert bool((np.abs(y.astype(np.float64) - y64) <= by + near * slack).all())
    s64 = (s0.astype(np.float64) + y64) * float(np.float32(scale))
    assert bool((np.abs(s.astype(np.float64) - s64) <= bs + near * slack * abs(scale)).all())
    # the noise of a row has length eps wherever p is not zero, up to the bound
    p, _ = L.propagate32(g, x)
    full = (p != 0).all(1)
    assert bool(full.any())
    length = np.sqrt(((y.astype(np.float64) - p.astype(np.float64)) ** 2).sum(1))
    # |y - p| differs from the exact noise by the rounding of the final addition (u |y|) on top of the noise's own error
    tol = np.sqrt((((by - L.propagate_bound(g, x)[0]) + U_ABS(y)) ** 2).sum(1))
    assert bool((np.abs(length - float(np.float32(eps)))[full] <= tol[full]).all())
    assert bool((y[g.deg == 0] == 0).all()) and not bool(np.signbit(y[g.deg == 0]).any()), 'a row without neighbours stays +0'
    # eps = 0 is the clean propagation, bit for bit; rows outside a range are zeros / untouched
    y0, s0b = R.propagate_noise32(g, x, 0.0, seed, stream, s0, scale)
    yc, sc = L.propagate32(g, x, s0, scale)
    assert np.array_equal(L.bits(y0), L.bits(yc)) and np.array_equal(L.bits(s0b), L.bits(sc))
    part, spart = R.propagate_noise32(g, x, eps, seed, stream, s0, scale, rows=(2, g.n - 1))
    assert np.array_equal(L.bits(part[2:g.n - 1]), L.bits(y[2:g.n - 1])) and not part[:2].any() and not part[g.n - 1:].any()
    assert np.array_equal(L.bits(spart[2:g.n - 1]), L.bits(s[2:g.n - 1])) and np.array_equal(spart[:2], s0[:2])


def U_ABS(y):
    return L.U * np.abs(np.asarray(y, dtype=np.float64))


@pytest.mark.parametrize('n_layers,keep', [(1, 1), (3, 1), (3, 3), (3, None), (2, 2)])
def test_horner_backward_against_float64_autograd(n_layers, keep):
    g = L.world(5, 64)
    d = 6
    e0 = torch.tensor(L.table(g.n, d, 3), dtype=torch.float64, requires_grad=True)
    w1, w2 = torch.tensor(L.table(g.n, d, 4), dtype=torch.float64), torch.tensor(L.table(g.n, d, 5), dtype=torch.float64)
    ls = R.layers_torch(torch.from_numpy(g.a_hat()), e0, n_layers, 0.1, 7, 2, 1, torch.float64)
    loss = ((sum(ls) / n_layers) * w1).sum()
    if keep is not None:
        loss = loss + (ls[keep - 1] * w2).sum()
    loss.backward()
    want = R.horner64(g, w1.numpy(), w2.numpy() if keep is not None else 0.0, n_layers, keep)
    scale = np.abs(want).max()
    assert float(np.abs(e0.grad.numpy() - want).max()) <= 1e-13 * scale
    # and the layers themselves: the same as the numpy form
    m, kept = R.mean64(g, e0.detach().numpy(), n_layers, 0.1, 7, 2, 1, keep)
    assert float(np.abs((sum(ls) / n_layers).detach().numpy() - m).max()) <= 1e-14
    assert (kept is None) == (keep is None)


def test_mean32_against_mean64():
    g = L.world(5, 64)
    e0 = L.table(g.n, 8, 3)
    m32, k32 = R.mean32(g, e0, 3, 0.1, 5, 1, 0, 2)
    m64, k64 = R.mean64(g, e0, 3, 0.1, 5, 1, 0, 2)
    assert float(np.abs(m32 - m64).max()) <= 1e-5 and float(np.abs(k32 - k64).max()) <= 1e-5
    clean, _ = R.mean32(g, e0, 3, 0.0, 5, 1, 0)
    with_layer_0 = L.mean64(g, e0, 3)
    assert float(np.abs(clean - (with_layer_0 * 4 - e0) / 3).max()) <= 1e-5, 'the clean table is the mean of the layers 1 .. L'


def test_the_float64_model_counts_distinct_rows():
    g, uw, iw, u, i, labels = L.model_world(8)
    for kind in ('simgcl', 'xsimgcl'):
        ref = R.model_torch(kind, g, uw, iw, u, i, labels, 2, torch.float64, keep_layer=2)
        assert ref['n_users'] == len(np.unique(u)) < len(u) and ref['n_items'] == len(np.unique(i[:, 0]))
        assert float(ref['reg_loss']) > 0 and np.isfinite(float(ref['loss']))
        off = R.model_torch(kind, g, uw, iw, u, i, labels, 2, torch.float64, cl_weight=0.0, keep_layer=2)
        assert float(off['reg_loss']) == 0 and not torch.equal(off['user_embeddings.weight'], ref['user_embeddings.weight'])


def test_constructors_refuse_and_the_registry_resolves():
    import sibrar_amd as S
    g = L.world(5, 64)
    for cls in (S.SimGCL, S.XSimGCL):
        for kw, text in (({'eps': -0.1}, 'eps'), ({'tau': 0.0}, 'tau'), ({'tau': -1.0}, 'tau'), ({'cl_weight': -1.0}, 'cl_weight'),
                         ({'n_layers': 0}, 'n_layers'), ({'n_layers': 64}, 'n_layers'), ({'eps': float('nan')}, 'eps'),
                         ({'seed': -1}, 'seed')):
            with pytest.raises(ValueError, match=text):
                cls(5, 64, g.m, **kw)
        with pytest.raises(ValueError, match='training matrix'):
            cls(5, 64, None)
    for keep in (0, 3):
        with pytest.raises(ValueError, match='keep_layer'):
            S.XSimGCL(5, 64, g.m, n_layers=2, keep_layer=keep)
    assert S.ALGORITHMS['simgcl'] is S.SimGCL and S.ALGORITHMS['xsimgcl'] is S.XSimGCL
    a, b = S.SimGCL(5, 64, g.m), S.XSimGCL(5, 64, g.m)
    assert (a.n_layers, a.eps, a.cl_weight, a.tau, a.seed, a.keep_layer) == (3, 0.1, 0.2, 0.2, 0, None)
    assert (b.n_layers, b.eps, b.cl_weight, b.tau, b.seed, b.keep_layer) == (2, 0.1, 0.2, 0.2, 0, 1)
    assert sorted(a.state_dict()) == sorted(b.state_dict()) == ['item_embeddings.weight', 'user_embeddings.weight']
    ds = S.SyntheticDataset(30, 20, 200, seed=1, n_negative_samples=2)
    net = S.ALGORITHMS['xsimgcl'].build_from_conf({'embedding_dim': 8, 'n_layers': 3, 'keep_layer': 2, 'eps': 0.2, 'seed': 9}, ds)
    assert isinstance(net, S.XSimGCL) and (net.embedding_dim, net.n_layers, net.keep_layer, net.eps, net.seed) == (8, 3, 2, 0.2, 9)
    net = S.ALGORITHMS['simgcl'].build_from_conf({'cl_weight': 0.5, 'tau': 0.1}, ds)
    assert isinstance(net, S.SimGCL) and (net.embedding_dim, net.n_layers, net.cl_weight, net.tau) == (64, 3, 0.5, 0.1)
    for step, view, layer in ((0, 4, 1), (0, 0, 64), (-1, 0, 1)):
        with pytest.raises(ValueError, match='noise_stream_id'):
            S.ops.noise_stream_id(step, view, layer)
    assert S.ops.noise_stream_id(3, 2, 5) == R.stream_id(3, 2, 5) == 3 * 256 + 2 * 64 + 5
