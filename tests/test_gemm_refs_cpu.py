"""The criteria of tests/gemm_ref.py on CPU arithmetic only: a torch emulation of the bf16-split product (three planes, six terms, fp32
accumulation in a shuffled order) and a float32 torch.matmul as the fp32-pipe stand-in must stay inside the derived bounds and
reproduce every exact family bit for bit; each mutation of the emulation (a dropped k index, a dropped plane term, two swapped
gathered rows, a column written past N) must be rejected by the criterion named in the test id. No GPU."""
import itertools

import numpy as np
import pytest
import torch

import gemm_ref as R
from hip_testutil import U32

TERMS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))      # the kernels' six kept terms, smallest first (gemm_split_f32.hip: mult_half)
M, N, K, N_TABLE = 24, 20, 128, 9


def bf16_rne(x):
    return x.bfloat16().float()                                # torch converts with round-to-nearest-even, as sp_pack does


def split3(x):
    x0 = bf16_rne(x)
    r1 = x - x0
    x1 = bf16_rne(r1)
    return x0, x1, bf16_rne(r1 - x1)


def emu_split_nt(a, b, bias, seed, drop_terms=(), drop_k=None):
    """sum over (k, kept term) of a_i[:, k] b_j[:, k]^T (+ bias) in float32, one rounding per addition, in a shuffled order"""
    ap, bp = split3(a), split3(b)
    items = [(k, i, j) for k in range(a.shape[1]) if k != drop_k for (i, j) in TERMS if (i, j) not in drop_terms]
    if bias is not None:
        items.append(None)
    rng = np.random.default_rng(seed)
    acc = torch.zeros(a.shape[0], b.shape[0])
    for q in rng.permutation(len(items)):
        it = items[q]
        acc = acc + (bias[None, :] if it is None else torch.outer(ap[it[1]][:, it[0]], bp[it[2]][:, it[0]]))
    return acc


def emu_f32_nt(a, b, bias):
    out = a @ b.t()
    return out if bias is None else out + bias[None, :]


def operands(fam, seed=3):
    """NT operands in gathered storage: A table [N_TABLE, K] read through a_idx (heavy repeats), B [N, K], padded leading dimensions"""
    tbl, b = R.family(fam, (N_TABLE, K), 1, (N, K), 1, seed)
    bias = {'rand6': R.gen_rand6((N,), seed + 2), 'ints': R.gen_int_bias(N, seed + 2)}.get(fam)
    a_idx = np.random.default_rng(seed).integers(0, N_TABLE, size=M)
    a_idx[:2] = (0, 1)                                         # two different rows in front: the swap mutation has something to swap
    lda, ldb = K + 4, K + 1
    A = torch.zeros(N_TABLE * lda)
    torch.as_strided(A, (N_TABLE, K), (lda, 1)).copy_(tbl)
    B = torch.zeros(N * ldb)
    torch.as_strided(B, (N, K), (ldb, 1)).copy_(b)
    return A, lda, a_idx, B, ldb, bias, tbl, b


def judge(fam, got, ref, S, bound_fn, what):
    if fam == 'rand6':
        R.check_bound(got, ref, bound_fn(S, K), f'{what} [bound on rand6]')
    else:
        R.check_exact(got, ref, f'{what} [exact family {fam}]')


@pytest.mark.parametrize('fam', ('rand6',) + R.FAMILIES_EXACT)
def test_standins_pass_every_criterion(fam):
    A, lda, a_idx, B, ldb, bias, tbl, b = operands(fam)
    ref, _, S = R.ref_nt(A, lda, a_idx, B, ldb, bias, M, N, K)
    a = tbl[torch.as_tensor(a_idx)]
    for seed in (0, 1):
        judge(fam, emu_split_nt(a, b, bias, seed), ref, S, R.bound_split, 'bf16-split emulation')
    judge(fam, emu_f32_nt(a, b, bias), ref, S, R.bound_f32, 'float32 matmul')


def test_rand6_operands_span_six_decades_and_bounds_have_the_stated_size():
    x = R.gen_rand6((4096,), 0).abs()
    assert float(x.min()) < 2e-3 and float(x.max()) > 5e2
    assert abs(R.gamma(K + 2) / ((K + 2) * U32) - 1) < 1e-4 and abs(R.gamma(6 * K + 8) / ((6 * K + 8) * U32) - 1) < 1e-4
    assert R.gamma(6 * K + 8) * R.F_SPLIT > 2.0 ** -15 > 2.0 ** -17      # why the random family cannot see a third-plane term


MUTATIONS = {
    # name: (family whose criterion rejects it, kwargs of the emulation, what else changes)
    'drop_one_k__rejected_by_ints': ('ints', dict(drop_k=77), None),
    'drop_term_02__rejected_by_onehot_full_a': ('onehot_full_a', dict(drop_terms=((0, 2),)), None),
    'drop_term_20__rejected_by_onehot_full_b': ('onehot_full_b', dict(drop_terms=((2, 0),)), None),
    'drop_term_11__rejected_by_onehot_two_plane_a': ('onehot_two_plane_a', dict(drop_terms=((1, 1),)), None),
    'drop_term_11__rejected_by_onehot_two_plane_b': ('onehot_two_plane_b', dict(drop_terms=((1, 1),)), None),
    'swap_two_gathered_rows__rejected_by_ints': ('ints', {}, 'swap'),
}


@pytest.mark.parametrize('name', sorted(MUTATIONS))
def test_mutation_is_rejected(name):
    fam, kw, extra = MUTATIONS[name]
    A, lda, a_idx, B, ldb, bias, tbl, b = operands(fam)
    ref, _, S = R.ref_nt(A, lda, a_idx, B, ldb, bias, M, N, K)
    idx = a_idx.copy()
    if extra == 'swap':
        idx[[0, 1]] = idx[[1, 0]]
    got = emu_split_nt(tbl[torch.as_tensor(idx)], b, bias, 0, **kw)
    with pytest.raises(AssertionError, match=f'exact family {fam}'):
        judge(fam, got, ref, S, R.bound_split, name)
    judge(fam, emu_split_nt(tbl[torch.as_tensor(a_idx)], b, bias, 0), ref, S, R.bound_split, 'unmutated')     # and only the mutation


@pytest.mark.parametrize('term', ((0, 2), (2, 0), (1, 1)))
def test_the_random_bound_alone_does_not_see_a_dropped_plane_term(term):
    """the reason for the exact families: a third-plane term is 2^-17 of a product, the worst-case bound at K = 128 about 2^-14 S"""
    A, lda, a_idx, B, ldb, bias, tbl, b = operands('rand6')
    ref, _, S = R.ref_nt(A, lda, a_idx, B, ldb, bias, M, N, K)
    got = emu_split_nt(tbl[torch.as_tensor(a_idx)], b, bias, 0, drop_terms=(term,))
    assert R.check_bound(got, ref, R.bound_split(S, K), 'mutated, rand6') <= 1.0


def test_mutation_write_one_column_past_n__rejected_by_the_guard_check():
    A, lda, a_idx, B, ldb, bias, tbl, b = operands('ints')
    out = emu_split_nt(tbl[torch.as_tensor(a_idx)], b, bias, 0)
    c_idx = np.random.default_rng(1).permutation(M + 5)[:M]           # scatter into a larger C
    good, bad = R.HostBuf(M + 5, N, N + 3), R.HostBuf(M + 5, N, N + 3)
    good.view()[c_idx] = out
    bad.view(N + 1)[c_idx] = torch.cat([out, out[:, :1]], 1)         # the mutation: column N of every addressed row
    ref, _, _ = R.ref_nt(A, lda, a_idx, B, ldb, bias, M, N, K)
    R.check_exact(good.check_untouched(c_idx, 'right kernel')[c_idx], ref, 'right kernel [exact family ints]')
    with pytest.raises(AssertionError, match='guard check'):
        bad.check_untouched(c_idx, 'column past N')
    worse = R.HostBuf(M + 5, N, N + 3)
    worse.view()[c_idx] = out
    worse.view()[[r for r in range(M + 5) if r not in set(c_idx.tolist())][0]] = 0.0       # a row that c_idx does not name
    with pytest.raises(AssertionError, match='guard check'):
        worse.check_untouched(c_idx, 'row outside c_idx')


def test_int_family_is_exact_up_to_the_longest_reduction_on_the_gpu():
    assert R.INT_MAX_ABS ** 2 * R.K_MAX_GPU + R.INT_BIAS_MAX < 2 ** 24
    a, b = R.family('ints', (4, 4096), 1, (4, 4096), 1, 0)
    assert float(a.abs().max()) == R.INT_MAX_ABS and float(b.abs().max()) == R.INT_MAX_ABS
    assert float(R.gen_int_bias(4096, 0).abs().max()) == R.INT_BIAS_MAX
    assert all(torch.equal(p, z) for x in (a, b) for p, z in zip(split3(x)[1:], (torch.zeros_like(x),) * 2))   # first bf16 plane only


def test_split_constants_of_the_docstring():
    x = torch.cat([R.gen_rand6((1 << 16,), 0), R.gen_full24((1 << 16,), 1), torch.randn(1 << 16, generator=torch.Generator().manual_seed(2))])
    x0, x1, x2 = split3(x)
    assert torch.equal(x0.double() + x1.double() + x2.double(), x.double())                 # the split is exact
    ax = x.double().abs()
    assert bool((x1.double().abs() <= 2.0 ** -8 * ax).all()) and bool((x2.double().abs() <= 2.0 ** -16 * ax).all())
    assert bool((x0.double().abs() <= (1 + 2.0 ** -8) * ax).all())
    kept = (1 + 2.0 ** -8) ** 2 + 2 * (1 + 2.0 ** -8) * 2.0 ** -8 + 2 * (1 + 2.0 ** -8) * 2.0 ** -16 + 2.0 ** -16
    assert kept < R.F_SPLIT and abs(kept - (1 + 2.0 ** -6 + 3 * 2.0 ** -15 + 2.0 ** -23)) < 1e-15
    y = R.gen_full24((1 << 16,), 3)                                                             # any order of the planes is exact
    for perm in itertools.permutations(split3(y)):
        assert torch.equal((perm[0] + perm[1]) + perm[2], y)
    t0, t1, t2 = split3(R.gen_two_plane((4096,), 4))
    assert bool((t1 != 0).all()) and not bool(t2.any()) and bool((t1.abs() == t0.abs() * 2.0 ** -10).all())


def test_references_against_an_independent_einsum_formulation():
    g = torch.Generator().manual_seed(5)
    m, n, k, ta, tb = 7, 5, 11, 4, 6
    lda, ldb = 13, 14
    A, B = torch.randn(64 * lda, generator=g), torch.randn(64 * ldb, generator=g)
    bias = torch.randn(n, generator=g)
    ai = np.array([3, 0, 0, 2, 3, 3, 1])
    at = lambda r, c: float(A[r * lda + c])
    bt = lambda r, c: float(B[r * ldb + c])
    # NT
    a2 = torch.tensor([[at(ai[i], j) for j in range(k)] for i in range(m)], dtype=torch.float64)
    b2 = torch.tensor([[bt(i, j) for j in range(k)] for i in range(n)], dtype=torch.float64)
    for act in range(5):
        out, pre, S = R.ref_nt(A, lda, ai, B, ldb, bias, m, n, k, act)
        want = torch.einsum('mk,nk->mn', a2, b2) + bias.double()
        assert torch.allclose(pre, want, rtol=1e-14, atol=1e-14)
        assert torch.allclose(S, torch.einsum('mk,nk->mn', a2.abs(), b2.abs()) + bias.double().abs(), rtol=1e-14)
        wact = {0: want, 1: want.clamp_min(0), 2: torch.tanh(want), 3: torch.sigmoid(want), 4: torch.nn.functional.selu(want)}[act]
        # (selu: the reference uses the kernels' fp32-rounded constants, torch the float64 ones: 3e-8 relative)
        assert torch.allclose(out, wact, rtol=1e-7 if act == 4 else 1e-12, atol=1e-14)
    # NN
    b2 = torch.tensor([[bt(i, j) for j in range(n)] for i in range(k)], dtype=torch.float64)
    out, _, S = R.ref_nn(A, lda, ai, B, ldb, m, n, k)
    assert torch.allclose(out, torch.einsum('mk,kn->mn', a2, b2), rtol=1e-14, atol=1e-14)
    assert torch.allclose(S, torch.einsum('mk,kn->mn', a2.abs(), b2.abs()), rtol=1e-14)
    # TN with both row maps
    ak, bk = np.array([1, 1, 3, 0, 2, 2, 2, 3, 0, 1, 3]) % ta, np.array([5, 4, 4, 0, 1, 2, 3, 5, 5, 0, 2]) % tb
    a2 = torch.tensor([[at(ak[i], j) for j in range(m)] for i in range(k)], dtype=torch.float64)
    b2 = torch.tensor([[bt(bk[i], j) for j in range(n)] for i in range(k)], dtype=torch.float64)
    out, _, S = R.ref_tn(A, lda, ak, B, ldb, bk, m, n, k)
    assert torch.allclose(out, torch.einsum('km,kn->mn', a2, b2), rtol=1e-14, atol=1e-14)
    assert torch.allclose(S, torch.einsum('km,kn->mn', a2.abs(), b2.abs()), rtol=1e-14)
    out0, _, _ = R.ref_tn(A, lda, None, B, ldb, None, m, n, k)
    assert torch.allclose(out0, torch.as_strided(A, (k, m), (lda, 1)).double().t() @ torch.as_strided(B, (k, n), (ldb, 1)).double())


@pytest.mark.parametrize('act', (2, 3, 4))
def test_activation_bounds_hold_for_float32_evaluation(act):
    """float32 torch activations of a float32 pre-activation inside the propagated bound (the fp32-pipe stand-in with an epilogue)"""
    A, lda, a_idx, B, ldb, bias, tbl, b = operands('rand6')
    scale = 1e-3                                               # pre-activations of a few units, where the activations are not saturated
    ref, pre, S = R.ref_nt(A * scale, lda, a_idx, B, ldb, bias * scale, M, N, K, act)
    pre32 = emu_f32_nt((tbl * scale)[torch.as_tensor(a_idx)], b, bias * scale)
    got = {2: torch.tanh, 3: torch.sigmoid, 4: torch.nn.functional.selu}[act](pre32)
    assert R.check_bound(got, ref, R.bound_f32(S, K, ref, pre, act), f'act {act}') <= 1.0


def test_gemm_f32_mode2_with_k0_returns_ok_on_the_host():
    """sbr_gemm_f32(mode 2, K = 0) used to divide by zero on the host (sbr_cdiv(K, k_chunk) with k_chunk = 0); it returns SBR_OK before
    any launch, so the call needs no device: the operand pointers are never dereferenced. Like the library tests of test_host_cpu.py it
    needs the built libsibrar_hip.so (build() of __graft_entry__.py): on an unbuilt tree it fails with SibrarHipError, 'is missing'"""
    from hip_testutil import _L
    buf = torch.zeros(64)
    p = buf.data_ptr()
    lib = _L().lib()
    before = lib.sbr_nondeterministic_launches()
    _L().call('sbr_gemm_f32', 2, p, 8, None, p, 8, None, None, p, 8, None, 8, 8, 0, 0, 1, None)
    assert bool((buf == 0).all())
    assert lib.sbr_nondeterministic_launches() == before           # nothing was launched, so nothing counts as arrival-order work
    with pytest.raises(_L().SibrarHipError, match='accumulate_atomic=1'):          # the refusal of mode 2 without accumulate_atomic still comes first
        _L().call('sbr_gemm_f32', 2, p, 8, None, p, 8, None, None, p, 8, None, 8, 8, 0, 0, 0, None)
