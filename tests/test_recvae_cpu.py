"""tests/recvae_ref.py against itself, without a GPU, at the shapes of tests/test_hip_swish_ln.py and tests/test_hip_prior_kl.py: the
closed-form float64 forward and backward formulas (the value halves of the bound pairs) against float64 autograd of the definitions; the
float32 restatement in the kernels' order inside the derived bound, the measured ratio printed; the LayerNorm invariants; the
log-sum-exp at the extremes; the float32-CPU error of the model, which tests/test_hip_recvae.py takes 8 times as its allowance; and the
package's side that needs no GPU (the registry, the constructor's refusals, the declared entries, the autoencoders' shared initialiser)."""
import math
import os
import re

import numpy as np
import pytest
import torch

import recvae_ref as R

ENTRIES = ('sbr_swish_ln_fwd', 'sbr_swish_ln_bwd', 'sbr_swish_ln_slabs', 'sbr_prior_kl_fwd', 'sbr_prior_kl_bwd')
SHAPES_H = [(B, H) for H in R.H_SIZES for B in R.BATCHES]
SHAPES_L = [(B, L) for L in R.L_SIZES for B in R.BATCHES]
CLOSE = 1e-9             # float64 closed form against float64 autograd, relative to the largest magnitude of the output


def close64(got, want, what):
    scale = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    assert err <= CLOSE * scale, f'{what}: closed form and autograd differ by {err} at scale {scale}'


def variants(r, dh, dr):
    """(r_in, dh, dr_out): the running sum present and NULL, either gradient NULL"""
    return [(r, dh, dr), (None, dh, dr), (r, dh, None), (r, None, dr), (None, dh, None)]


@pytest.mark.parametrize('B,H', SHAPES_H)
def test_swish_ln_closed_forms_and_restatement(B, H):
    a, r, gamma, beta, dh, dr = R.swish_ln_case(B, H, 0)
    worst = {}
    for r_in, g_h, g_r in variants(r, dh, dr):
        bound = R.swish_ln_bound(a, r_in, gamma, beta, R.LN_EPS, g_h, g_r)
        auto = R.swish_ln_autograd(a, r_in, gamma, beta, g_h, g_r)
        got = R.swish_ln32(a, r_in, gamma, beta, R.LN_EPS, g_h, g_r)
        for k in ('h', 'r_out', 'da', 'dr_in', 'dgamma', 'dbeta'):
            if auto[k] is None:
                continue
            if not (H == 1 and k == 'da'):                                # H = 1: d = 0 exactly, the closed form is 0 and autograd's 0 too
                close64(bound[k].v, auto[k], k)
            worst[k] = max(worst.get(k, 0.0), R.ratio(got[k], bound[k]))
    print(f'B = {B}, H = {H}: float32 restatement, largest error / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize('B,L', SHAPES_L)
def test_prior_kl_closed_forms_and_restatement(B, L):
    mu, logvar, eps, mu_old, logvar_old, weight, dz = R.prior_kl_case(B, L, 0)
    worst = {}
    for g_z, up in ((dz, 0.7), (None, 1.0), (dz, 0.0)):
        scale = 1.0 / B
        bound = R.prior_kl_bound(mu, logvar, eps, mu_old, logvar_old, weight, g_z, up, scale)
        auto = R.prior_kl_autograd(mu, logvar, eps, mu_old, logvar_old, weight, g_z, up, scale)
        got = R.prior_kl32(mu, logvar, eps, mu_old, logvar_old, weight, g_z, up, scale)
        for k in ('z', 'row_kl', 'dmu', 'dlogvar'):
            scale_k = max(1.0, float(np.abs(auto[k]).max()))
            assert float(np.abs(bound[k].v - auto[k]).max()) <= 1e-7 * scale_k, k      # log q's two paths cancel in autograd: 1e-16 times 1 / exp(logvar)
            worst[k] = max(worst.get(k, 0.0), R.ratio(got[k], bound[k]))
        assert np.array_equal(got['z'], R.z32(mu, logvar, eps))
    print(f'B = {B}, L = {L}: float32 restatement, largest error / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_layernorm_invariants():
    rng = np.random.default_rng(0)
    H = 65
    gamma, beta = (1 + rng.standard_normal(H)).astype(np.float32), rng.standard_normal(H).astype(np.float32)
    const = np.full((3, H), 0.75, dtype=np.float32)
    out = R.swish_ln32(const, None, gamma, beta)
    assert np.array_equal(out['h'], np.tile(beta, (3, 1))), 'a constant row gives beta'
    assert np.array_equal(out['rstd'], np.full(3, np.float32(1) / np.sqrt(np.float32(R.LN_EPS)), dtype=np.float32))
    # shifting a row's pre-LayerNorm values changes nothing: LN(y + c) = LN(y) in the float64 definition
    y = torch.from_numpy(rng.standard_normal((4, H)))
    g, b = R.t64(gamma), R.t64(beta)

    def ln(v):
        d = v - v.mean(1, keepdim=True)
        return d / torch.sqrt((d * d).mean(1, keepdim=True) + R.LN_EPS) * g + b
    assert float((ln(y + 1000.0) - ln(y)).abs().max()) <= 1e-10
    # and a one-pass variance fails the bound on the large-mean row, which the two-pass restatement meets
    a, _, gamma, beta, _, _ = R.swish_ln_case(3, 600, 0, with_sum=False)
    bound = R.swish_ln_bound(a, None, gamma, beta)
    assert R.ratio(R.swish_ln32(a, None, gamma, beta)['h'], bound['h']) <= 1.0
    yy = (a * (1 / (1 + np.exp(-a)))).astype(np.float32)
    m = yy.mean(1, dtype=np.float32)
    var1 = (yy * yy).mean(1, dtype=np.float32) - m * m
    h1 = (yy - m[:, None]) / np.sqrt(np.maximum(var1, 0) + np.float32(R.LN_EPS))[:, None] * gamma + beta
    assert R.ratio(h1[1:2].astype(np.float32), R.E(bound['h'].v[1:2], bound['h'].e[1:2])) > 1.0, 'the large-mean row does not tell the two apart'


def test_logsumexp_stays_finite_at_the_extremes():
    z = np.array([[-50.0, 50.0, 0.0, 1e-5, 49.0, -3.0]], dtype=np.float32)
    zero = np.zeros_like(z)
    for lvo in (-20.0, 0.0, 10.0):
        for mo in (0.0, 50.0):
            out = R.prior_kl32(z, zero, zero, zero + np.float32(mo), zero + np.float32(lvo), np.ones(1, dtype=np.float32), None, 1.0, 1.0)
            assert np.isfinite(out['row_kl']).all() and np.isfinite(out['dmu']).all() and np.isfinite(out['dlogvar']).all(), (lvo, mo)
            bound = R.prior_kl_bound(z, zero, zero, zero + np.float32(mo), zero + np.float32(lvo), np.ones(1, dtype=np.float32), None, 1.0, 1.0)
            assert R.ratio(out['row_kl'], bound['row_kl']) <= 1.0 and R.ratio(out['dmu'], bound['dmu']) <= 1.0
            mx, e, se = R._mix32(z, zero + np.float32(mo), zero + np.float32(lvo))
            assert (se >= 1).all() and (se <= 3).all(), 'the largest exponent is 0'


def test_model_float32_error_on_the_cpu():
    out64, g64, out32, g32, *_ = R.model_errors()
    out64, out32 = [t.detach() for t in out64], [t.detach() for t in out32]
    errs = {'loss': abs(float(out32[0]) - float(out64[0]))}
    for k in R.PARAMS:
        errs['grad ' + k] = float((g32[k].double() - g64[k]).abs().max())
        assert float(g64[k].abs().max()) > 0, f'{k} has no gradient: the comparison would be empty'
    print('float32 torch on the CPU against float64: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    print(f'loss {float(out64[0]):.6f} (nll {float(out64[1]):.6f}, kld {float(out64[2]):.6f}); largest gradient error {max(v for k, v in errs.items() if k != "loss"):.3e}')
    assert all(v > 0 for v in errs.values()), 'a float32 error of exactly 0 would make the GPU test\'s allowance 0'
    assert errs['loss'] <= 1e-4 * abs(float(out64[0]))


@pytest.mark.parametrize('seed', [0, 5])
def test_the_shared_initialiser_draws_in_the_stated_order(seed):
    """row_autoencoder.init_weights on the Mult-VAE, Mult-DAE and RecVAE tables at (n_items, hidden, latent) = (7, 4, 3): a matrix
    [out, in] is randn * sqrt(2 / (out + in)), a vector randn * 0.001, drawn in the table's order from one generator; the first layer
    is column-major; the LayerNorm constants draw nothing. The expected tensors are written out with torch.randn."""
    from importlib import import_module
    import sibrar_amd as S
    pkg = S.ops.__name__.rsplit('.', 1)[0]
    init_weights, multvae = import_module(pkg + '.row_autoencoder').init_weights, import_module(pkg + '.multvae')
    I, H, L = 7, 4, 3

    def gen():
        return torch.Generator().manual_seed(seed)

    def mat(g, out, inp):
        return torch.randn(out, inp, generator=g) * math.sqrt(2.0 / (out + inp))

    def vec(g, n):
        return torch.randn(n, generator=g) * 0.001

    for cls, code in ((S.MultVAE, 2 * L), (S.MultDAE, L)):
        g = gen()
        want = {}
        for layer, (out, inp) in zip(('enc1', 'enc2', 'dec1', 'dec2'), ((H, I), (code, H), (H, L), (I, H))):
            want['w_' + layer] = mat(g, out, inp)
            want['b_' + layer] = vec(g, out)
        got = init_weights(cls.shapes(I, H, L), gen(), (cls.INPUT,), cls.CONSTANTS)
        assert tuple(got) == tuple(want) == multvae.PARAMS
        for k in want:
            assert got[k].dtype == torch.float32 and torch.equal(got[k], want[k]), f'{cls.__name__}: {k}'
        assert got['w_enc1'].t().is_contiguous() and got['w_dec2'].is_contiguous()
        net = multvae.AutoencoderWeights(I, H, L, code, seed)
        assert [k for k, _ in net.named_parameters()] == list(want) and all(torch.equal(getattr(net, k), want[k]) for k in want)
        assert net.w_enc1.t().is_contiguous()

    g = gen()
    want = {}
    for k in range(1, 6):
        want[f'fc_w{k}'] = mat(g, H, I if k == 1 else H)
        want[f'fc_b{k}'] = vec(g, H)
        want[f'ln_w{k}'], want[f'ln_b{k}'] = torch.ones(H), torch.zeros(H)
    want['mu_w'], want['mu_b'] = mat(g, L, H), vec(g, L)
    want['logvar_w'], want['logvar_b'] = mat(g, L, H), vec(g, L)
    want['dec_w'], want['dec_b'] = mat(g, I, L), vec(g, I)               # the draw that follows logvar_b: the ln_* took none
    got = init_weights(S.RecVAE.shapes(I, H, L), gen(), (S.RecVAE.INPUT,), S.RecVAE.CONSTANTS)
    assert tuple(got) == tuple(want) == R.PARAMS
    for k in want:
        assert got[k].dtype == torch.float32 and torch.equal(got[k], want[k]), f'RecVAE: {k}'
    assert got['fc_w1'].t().is_contiguous() and got['fc_w2'].is_contiguous()
    assert S.RecVAE.PARTS == {'encoder': R.ENCODER_PARAMS, 'decoder': R.DECODER_PARAMS}


def test_package_side_without_a_gpu():
    import sibrar_amd as S
    assert S.ALGORITHMS['recvae'] is S.RecVAE and issubclass(S.RecVAE, S.ResidentMatrixAlgorithm)
    d = S.ALGORITHMS['recvae'].build_from_conf({}, None)
    assert (d.hidden, d.latent, d.dropout, d.gamma, d.beta, d.lr, d.batch_size, d.n_epochs, d.n_enc_epochs, d.n_dec_epochs, d.weight_decay, d.seed) == \
        (600, 200, 0.5, 0.005, None, 5e-4, 500, 50, 3, 1, 0., 0)
    with pytest.raises(ValueError, match='gamma and beta'):
        S.RecVAE(gamma=None, beta=None)
    with pytest.raises(ValueError, match='gamma is 0'):
        S.RecVAE(gamma=0)
    assert S.RecVAE(gamma=None, beta=0.2).beta == 0.2
    assert hasattr(S.ops, 'SwishLayerNormFn') and hasattr(S.ops, 'CompositePriorKLFn')
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sibrar_hip.h')).read()
    for entry in ENTRIES:
        params = re.search(r'\b' + entry + r'\s*\(([^)]*)\)\s*;', header).group(1)
        assert not re.search(r'\blong\s+ld\w*', params), f'{entry} takes a leading dimension'
