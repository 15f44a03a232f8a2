"""Mult-VAE / Mult-DAE without a GPU: the float64 definitions of the multinomial likelihood on hand-worked rows, the float64 model's
gradients against finite differences, and the planted world on which the GPU tests ask the package's models to beat popularity: here the
float64 reference reaches NDCG@10 >= 0.30 on it and popularity stays below 0.07, which is what gives the GPU condition (twice
popularity) its room. The entry the GPU tests pin is 'sbr_multinomial_nll_f32'."""
import math

import numpy as np
import pytest
import torch

import multvae_ref as R

ENTRY = 'sbr_multinomial_nll_f32'


def test_hand_worked_rows():
    # n_items = 1: lse = z, the loss of a positive is 0 and the gradient 0; of an empty row 0
    loss, lse, d = R.nll64([[2.5]], [[1]], 1.0)
    assert loss[0] == 0 and lse[0] == 2.5 and d[0, 0] == 0
    loss, lse, d = R.nll64([[2.5]], [[0]], 1.0)
    assert loss[0] == 0 and lse[0] == 2.5 and d[0, 0] == 0
    # a constant row c of I items with n positives: lse = c + log I, loss = n log I, d = gs (n / I - t)
    I, n, c = 8, 3, -1.75
    t = np.zeros((1, I))
    t[0, [1, 4, 6]] = 1
    loss, lse, d = R.nll64(np.full((1, I), c), t, 0.5)
    assert abs(lse[0] - (c + math.log(I))) < 1e-15 and abs(loss[0] - n * math.log(I)) < 1e-14
    assert np.allclose(d[0], 0.5 * (n / I - t[0]), rtol=0, atol=1e-15)
    # n = 0: zero loss and a zero gradient row whatever the logits; n = n_items: loss = I lse - sum z, the gradient sums to zero
    z = np.array([[0.3, -1.2, 2.0, 0.1]])
    loss, _, d = R.nll64(z, np.zeros((1, 4)), 1.0)
    assert loss[0] == 0 and not d.any()
    loss, lse, d = R.nll64(z, np.ones((1, 4)), 1.0)
    assert abs(loss[0] - (4 * lse[0] - z.sum())) < 1e-14 and abs(d.sum()) < 1e-14 and np.allclose(d[0], 4 * np.exp(z[0] - lse[0]) - 1)


def test_the_bound_is_positive_and_small_at_the_test_shapes():
    rng = np.random.default_rng(0)
    for I in (1, 65, 1027, 4100):
        z = rng.standard_normal((3, I)).astype(np.float32)
        t = (rng.random((3, I)) < 0.2).astype(np.float64)
        eloss, else_, ed = R.nll_bound(z, t, 1.0 / 3)
        assert (else_ > 0).all() and (else_ < 1e-4).all() and (ed >= 0).all() and float(ed.max()) < 1e-4 and (eloss >= 0).all()


@pytest.mark.parametrize('variational', [False, True])
def test_float64_model_gradients_against_finite_differences(variational):
    rng = np.random.default_rng(3)
    B, I, hidden, latent = 5, 11, 6, 3
    x = torch.from_numpy((rng.random((B, I)) < 0.4).astype(np.float64))
    x[0] = 0                                                            # a user without items: zero loss row
    eps = torch.from_numpy(rng.standard_normal((B, latent)))
    keep = torch.from_numpy(rng.random((B, I)) < 0.7)
    p = R.init_params(I, hidden, latent, variational, 1)
    with torch.no_grad():
        for v in p.values():
            v.mul_(8)                                                   # away from the linear regime of the tanh

    def f():
        return R.forward(p, x, variational, eps, keep, 0.3, 0.15)[0]

    f().backward()
    h = 1e-6
    for name, v in p.items():
        flat, g = v.data.view(-1), v.grad.view(-1)
        for k in rng.choice(flat.numel(), size=min(6, flat.numel()), replace=False):
            old = float(flat[k])
            flat[k] = old + h
            up = float(f().detach())
            flat[k] = old - h
            down = float(f().detach())
            flat[k] = old
            fd = (up - down) / (2 * h)
            assert abs(fd - float(g[k])) <= 1e-6 * max(1.0, abs(fd)), f'{name}[{k}]: autograd {float(g[k])}, finite difference {fd}'


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_planted_world_reference_beats_popularity(seed):
    train, held = R.planted_world(seed)
    assert train.shape == (R.N_USERS, R.N_ITEMS) and train.nnz == R.N_USERS * (R.PER_USER - R.HELD_OUT)
    pop = R.ndcg_at_10(R.popularity_scores(train), train, held)
    print(f'seed {seed}: popularity NDCG@10 {pop:.4f}')
    assert pop < 0.07
    for variational in (True, False):
        got = R.ndcg_at_10(R.train_reference(train, variational, seed, **R.SETTINGS), train, held)
        print(f'seed {seed}: {"Mult-VAE" if variational else "Mult-DAE"} float64 reference NDCG@10 {got:.4f}')
        assert got >= 0.30
