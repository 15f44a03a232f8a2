"""The references of tests/optim_ref.py on CPU arithmetic only: the float64 rules against torch.optim on float64 parameters; the fp32
restatement of the kernels inside the derived bounds on every input set that tests/test_hip_optim.py generates (the condition that
makes the bounds legitimate: the reference arithmetic alone passes them); and each listed wrong kernel — a mutation of the
restatement — outside the bounds on at least one of those input sets. No GPU."""
import numpy as np
import pytest
import torch

import optim_ref as O
import test_hip_optim as G


# ---- the rules against torch.optim -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['adamw', 'adam', 'adagrad'])
@pytest.mark.parametrize('lr,betas,eps,wd', [(1e-3, (0.9, 0.999), 1e-8, 1e-2), (3e-2, (0.5, 0.99), 1e-3, 0.3), (1e-2, (0.0, 0.9), 1e-12, 0.0),
                                              (1e-1, (0.99, 0.999), 1e-6, 1e-2)])
def test_rules_equal_torch_optim_in_float64(name, lr, betas, eps, wd):
    """six steps of torch.optim.{AdamW, Adam, Adagrad} on a float64 parameter == the rule fed with its own output, to 1e-13 of the
    magnitudes that form each quantity (the two differ in the order of a few float64 operations only)"""
    gen = torch.Generator().manual_seed(1)
    n = 500
    p0 = torch.randn(n, generator=gen, dtype=torch.float64)
    grads = [torch.randn(n, generator=gen, dtype=torch.float64) * 10.0 ** (s - 3) for s in range(6)]
    pt = torch.nn.Parameter(p0.clone())
    if name == 'adagrad':
        opt = torch.optim.Adagrad([pt], lr=lr, eps=eps, weight_decay=wd)
    else:
        opt = {'adamw': torch.optim.AdamW, 'adam': torch.optim.Adam}[name]([pt], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    p, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for s, g in enumerate(grads):
        pt.grad = g.clone()
        opt.step()
        st = opt.state[pt]
        if name == 'adagrad':
            (p, v), _ = O.adagrad_ref(p, g, v, lr, eps, wd)
            pairs = [(v, st['sum'], v)]
        else:
            (p, m, v), _ = O.adam_ref(0 if name == 'adamw' else 1, p, g, m, v, lr, betas[0], betas[1], eps, wd, s + 1)
            pairs = [(m, st['exp_avg'], m.abs() + g.abs() + wd * p0.abs()), (v, st['exp_avg_sq'], v)]
        pairs.append((p, pt.detach(), p.abs() + p0.abs() + lr / (1 - betas[0])))
        for mine, theirs, scale in pairs:
            assert bool(((mine - theirs).abs() <= 1e-13 * scale).all()), f'{name} step {s + 1}'


# ---- the restatement inside the bounds, the mutants outside --------------------------------------------------------------------
def _f32_step(opt, p, g, m, v, h, t, mutant=None):
    if opt == 2:
        return O.adagrad_f32(p, g, v, h[0], h[1], h[2], mutant)
    lr, wd, b1, b2, eps, step = h
    return O.adam_f32(opt, p, g, m, v, lr, b1, b2, eps, wd, step + t, mutant)


def _walk(case, mutant=None):
    """the steps of one GPU case -> per step and output (name, err / bound as a tensor over the elements); the unmutated restatement's
    output is the state of the next step, as the kernel's is on the GPU"""
    opt, n, h, seed, steps = case
    p, g, m, v = G.state(n, seed)
    out = []
    for t in range(steps):
        refs, bounds = G.rule(opt, p, g, m, v, h, t)
        got = _f32_step(opt, p, g, m, v, h, t, mutant)
        for o, r, b, nm in zip(got, refs, bounds, G.NAMES[opt]):
            assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(b).all()) and bool((b > 0).all()), f'{case}: no finite bound for {nm}'
            out.append((nm, (torch.from_numpy(o).double() - r).abs() / b))
        if steps > 1:
            clean = got if mutant is None else _f32_step(opt, p, g, m, v, h, t)
            p = torch.from_numpy(clean[0])
            m, v = (m, torch.from_numpy(clean[1])) if opt == 2 else (torch.from_numpy(clean[1]), torch.from_numpy(clean[2]))
            g = G.next_gradient(n, seed, t)
    return out


CASES = G.dense_cases()
SMALL = [c for c in CASES if c[1] <= 4100]


def test_the_cases_cover_what_the_gpu_tests_promise():
    assert {c[1] for c in CASES} >= set(G.SIZES) | {G.N_CAP_ELEMENT, G.N_CAP_QUAD}
    for opt in (0, 1):
        assert {c[2] for c in CASES if c[0] == opt} == set(G.HYPERS)
    assert {c[2] for c in CASES if c[0] == 2} == set(G.HYPERS_ADAGRAD)
    lr, wd, b1, b2, eps, step = (set(x) for x in zip(*G.HYPERS))
    assert wd == {0.0, 1e-2, 0.3} and b1 == {0.0, 0.5, 0.9, 0.99} and b2 == {0.9, 0.99, 0.999} and eps == {1e-12, 1e-8, 1e-3}
    assert step == {1, 2, 10, 1000, 10 ** 6} and 0.0 in lr and min(lr - {0.0}) == 1e-5 and max(lr) == 1e-1
    p, g, m, v = G.state(4100, 0)
    assert bool((g == 0).any()) and bool((G._bits(g) == -2 ** 31).any()) and bool((m == 0).any()) and bool((v == 0).any())
    tiny = 2.0 ** -126
    assert bool(((m != 0) & (m.abs() < tiny)).any()) and bool(((v != 0) & (v < tiny)).any()) and float(v[v > tiny].min()) < 1e-37
    assert 1e-6 <= float(g[g != 0].abs().min()) < 1e-5 and 10 < float(g.abs().max()) <= 1e2


@pytest.mark.parametrize('case', CASES, ids=lambda c: f'opt{c[0]}-n{c[1]}-seed{c[3]}')
def test_fp32_restatement_stays_inside_the_bound(case):
    worst = {}
    for nm, ratio in _walk(case):
        worst[nm] = max(worst.get(nm, 0.0), float(ratio.max()))
    print(f'restatement err / bound {case[:2]}: {worst}')
    assert all(w <= 1.0 for w in worst.values()), f'{case}: {worst}'


def _seen(mutant, opts):
    """the largest err / bound the mutant reaches on the small input sets of the optimizers ``opts``"""
    return max(float(torch.nan_to_num(ratio, nan=float('inf')).max()) for c in SMALL if c[0] in opts for _, ratio in _walk(c, mutant))


@pytest.mark.parametrize('mutant', O.MUTANTS_ADAM)
def test_wrong_adam_kernels_leave_the_bound(mutant):
    """1 - b2 evaluated in fp32; the bias correction one step early / late; eps under the root; decoupled decay and L2 term swapped
    between AdamW and Adam; the second moment fed with the gradient before wd p was added: each is outside the bound somewhere"""
    groups = {'v_from_the_gradient_without_wd_p': [(1,)], 'decay_kinds_swapped': [(0,), (1,)]}.get(mutant, [(0, 1)])   # the swap: seen from both sides
    for opts in groups:
        worst = _seen(mutant, opts)
        print(f'{mutant} on {opts}: worst err / bound {worst:.3g}')
        assert worst > 1.0, f'{mutant}: no input set of the GPU tests sees it (worst err / bound {worst:.3g})'


@pytest.mark.parametrize('mutant', O.MUTANTS_ADAGRAD)
def test_wrong_adagrad_kernels_leave_the_bound(mutant):
    worst = _seen(mutant, (2,))
    print(f'{mutant}: worst err / bound {worst:.3g}')
    assert worst > 1.0, f'{mutant}: no input set of the GPU tests sees it (worst err / bound {worst:.3g})'


def test_restatement_without_a_mutant_is_the_same_function():
    """(guards the mutant switch itself) mutant=None twice gives the same bits, and every mutant changes some bit"""
    p, g, m, v = G.state(1028, 3)
    lr, wd, b1, b2, eps, step = G.HYPERS[0]
    base = O.adam_f32(1, p, g, m, v, lr, b1, b2, eps, wd, step)
    again = O.adam_f32(1, p, g, m, v, lr, b1, b2, eps, wd, step)
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(base, again))
    for mutant in O.MUTANTS_ADAM:
        mut = O.adam_f32(1, p, g, m, v, lr, b1, b2, eps, wd, step, mutant)
        assert any(not np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(base, mut)), mutant


@pytest.mark.parametrize('kind', [0, 1])
@pytest.mark.parametrize('D', [1, 64, 65, 130])
def test_compounded_bound_holds_for_a_chain_of_fp32_steps(kind, D):
    """the deferred tests' criterion on their own table: T_STEPS dense fp32 steps chained (what a deferred row replays, bit for bit)
    against the float64 trajectory from the same start, within the bound that optim_ref propagates through e_in"""
    lr, b1, b2, eps, wd = G.H_ROWS
    _, p0, m0, v0, _, _ = G._rows_world(D, 11 * D + kind, zero_state_rows=slice(12, G.R_ROWS))
    got, ref, err = (p0, m0, v0), (p0.double(), m0.double(), v0.double()), None
    for t in range(1, G.T_STEPS + 1):
        grad = G.next_gradient(G.R_ROWS * D, D, t).view(G.R_ROWS, D) * (torch.arange(G.R_ROWS) % 3 == t % 3)[:, None]
        got = tuple(torch.from_numpy(x) for x in O.adam_f32(kind, got[0], grad, got[1], got[2], lr, b1, b2, eps, wd, t))
        ref, err = O.adam_ref(kind, ref[0], grad, ref[1], ref[2], lr, b1, b2, eps, wd, t, e_in=err)
    for o, r, b, nm in zip(got, ref, err, 'pmv'):
        print(f'chain kind {kind} D {D} {nm}: err / bound {O.check_bound(o, r, b, nm):.3f}')
