"""RecVAE on the GPU (recvae.py over ``ops.SwishLayerNormFn`` / 'sbr_swish_ln_fwd', 'sbr_swish_ln_bwd' and ``ops.CompositePriorKLFn`` /
'sbr_prior_kl_fwd', 'sbr_prior_kl_bwd'): one loss and all parameter gradients against the float64 model of tests/recvae_ref.py, within 8
times the error of the same network in float32 torch on the CPU; the alternation and the old encoder's independence of the optimizer's
flat buffer, bit for bit; fit, deterministic mode, model.npz, the evaluation hooks, predict, the registry."""
import functools
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import recvae_ref as R
from hip_testutil import DEV, S, _assert_bits

pytestmark = pytest.mark.gpu
CONF = dict(R.SETTINGS)


def _mod(name):
    return import_module(S().ops.__name__.rsplit('.', 1)[0] + '.' + name)


def arrays(m):
    return {k: getattr(m.encoder if k in R.ENCODER_PARAMS else m.decoder, k) for k in R.PARAMS}


def snapshot(tensors):
    return {k: v.detach().clone() for k, v in tensors.items()}


def prepared(seed=0, **kw):
    """a model on the planted world with its training state set up and no epoch run"""
    return S().RecVAE(seed=seed, device=DEV, n_epochs=0, **{**CONF, **kw}).fit(R.planted_world(0))


# ---- 1. against the float64 model ------------------------------------------------------------------------------------------------------------
def test_loss_and_gradients_against_float64():
    out64, g64, out32, g32, p64, old64, x, eps = R.model_errors()
    m = prepared()
    rv = _mod('recvae')
    assert rv.PARAMS == R.PARAMS and m.encoder.fc_w1.t().is_contiguous()
    with torch.no_grad():
        for k, v in arrays(m).items():
            v.copy_(p64[k].detach().float())
        for k in R.ENCODER_PARAMS:
            getattr(m.old, k).copy_(old64[k].float())
    users = torch.arange(R.N_USERS, device=DEV)
    loss, nll, kld, logits = m.loss(users, eps.float().to(DEV), dropout_seed=None, inplace=False)
    loss.backward()

    def check(name, got, ref64, ref32):
        tol = 8 * float((ref32.detach().double() - ref64.detach()).abs().max())
        err = float((got.detach().cpu().double() - ref64.detach()).abs().max())
        print(f'{name}: error {err:.3e}, 8 x float32-CPU error {tol:.3e}')
        assert err <= tol, f'{name}: {err} > {tol}'

    check('loss', loss, out64[0], out32[0])
    check('nll', nll, out64[1], out32[1])
    check('kld', kld, out64[2], out32[2])
    check('logits', logits, out64[3], out32[3])
    for k, v in arrays(m).items():
        check('grad ' + k, v.grad, g64[k], g32[k])
    with torch.no_grad():
        s64 = out64[4] @ p64['dec_w'].t() + p64['dec_b']
        s32 = (out32[4] @ p64['dec_w'].float().t() + p64['dec_b'].float())
    check('score rows (decoder(mu))', m._score_rows(users), s64, s32)


# ---- 2. the alternation and the old encoder -------------------------------------------------------------------------------------------------------
def test_alternation_and_the_old_encoder_hold_bit_for_bit():
    m = prepared(seed=1)
    enc0, dec0 = snapshot({k: v for k, v in arrays(m).items() if k in R.ENCODER_PARAMS}), snapshot({k: getattr(m.decoder, k) for k in R.DECODER_PARAMS})
    m.train_pass('encoder')
    for k in R.DECODER_PARAMS:
        _assert_bits(getattr(m.decoder, k).detach().cpu(), dec0[k].cpu(), f'an encoder pass moved {k}')
    assert all(not torch.equal(getattr(m.encoder, k).detach(), enc0[k]) for k in R.ENCODER_PARAMS), 'an encoder pass left an encoder array unchanged'
    for k in R.ENCODER_PARAMS:
        _assert_bits(getattr(m.old, k).cpu(), enc0[k].cpu(), f'the old encoder\'s {k} followed the encoder before update_prior()')
    m.update_prior()
    enc1 = snapshot({k: getattr(m.encoder, k) for k in R.ENCODER_PARAMS})
    flat = m._opt_enc.fp.flat
    for k in R.ENCODER_PARAMS:
        old = getattr(m.old, k)
        _assert_bits(old.cpu(), enc1[k].cpu(), f'after update_prior() the old encoder\'s {k} is the encoder\'s')
        assert not isinstance(old, torch.nn.Parameter) and not old.requires_grad
        assert not (flat.data_ptr() <= old.data_ptr() < flat.data_ptr() + 4 * flat.numel()), f'the old {k} lives in the optimizer\'s flat buffer'
    assert m.old.fc_w1.t().is_contiguous()
    m.train_pass('decoder')
    for k in R.ENCODER_PARAMS:
        _assert_bits(getattr(m.encoder, k).detach().cpu(), enc1[k].cpu(), f'a decoder pass moved {k}')
    assert all(not torch.equal(getattr(m.decoder, k).detach(), dec0[k]) for k in R.DECODER_PARAMS), 'a decoder pass left the decoder unchanged'
    # the aliasing test: one further encoder step moves the encoder and not the old encoder
    users = m._active[:16].contiguous()
    eps = torch.randn(16, m.latent, generator=torch.Generator().manual_seed(5)).to(DEV)
    m.loss(users, eps, dropout_seed=11)[0].backward()
    m._opt_enc.step()
    m._opt_enc.zero_grad()
    for k in R.ENCODER_PARAMS:
        _assert_bits(getattr(m.old, k).cpu(), enc1[k].cpu(), f'the old encoder\'s {k} followed an optimizer step')
        assert not torch.equal(getattr(m.encoder, k).detach(), enc1[k]), f'{k} did not move'


# ---- 3. fit, deterministic mode, persistence, evaluation ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fitted():
    train = R.planted_world(0)
    return S().RecVAE(seed=0, device=DEV, n_epochs=3, **CONF).fit(train), train


def test_a_three_epoch_fit_lowers_the_epoch_loss():
    m, _ = fitted()
    print('epoch losses', m.epoch_losses)
    assert len(m.epoch_losses) == 3 and all(np.isfinite(m.epoch_losses)) and m.epoch_losses[-1] < m.epoch_losses[0]


def test_two_fits_from_one_seed_give_the_same_bits_in_deterministic_mode():
    Sm = S()
    train = R.planted_world(0)
    prev = Sm.ops.set_deterministic(True)
    try:
        a, b = (Sm.RecVAE(seed=4, device=DEV, n_epochs=2, **CONF).fit(train) for _ in range(2))
    finally:
        Sm.ops.set_deterministic(prev)
    for (k, x), y in zip(arrays(a).items(), arrays(b).values()):
        assert torch.equal(x, y), f'{k} differs between two fits'
    assert a.epoch_losses == b.epoch_losses


def eval_view(train):
    n_users, n_items = train.shape
    held = np.asarray(train.argmax(1)).reshape(-1)                       # any labels: the evaluation only has to run
    holdout = sp.csr_matrix((np.ones(n_users), (np.arange(n_users), (held + 1) % n_items)), shape=train.shape)
    return SimpleNamespace(n_users=n_users, n_items=n_items, items_in_split=np.arange(n_items), users_in_split=np.arange(n_users),
                           n_items_in_split=n_items, n_users_in_split=n_users, user_sampling_matrix=holdout, exclude_data=train.astype(bool),
                           user_features={}, item_features={})


def test_evaluation_predict_and_persistence(tmp_path):
    Sm = S()
    m, train = fitted()
    view = eval_view(train)
    ev = Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=(10,)), dataset=view)
    res = Sm.evaluate_recommender_algorithm(m, type('L', (), {'dataset': view, 'batch_size': 32})(), ev, DEV)
    assert 0.0 <= res['ndcg@10'] <= 1.0
    u = torch.tensor([0, 5, 47, 17])
    i = torch.tensor([[0, 39, 3], [1, 2, 3], [20, 21, 22], [7, 7, 8]])
    rows = m._score_rows(u.to(DEV))
    _assert_bits(m.predict(u, i).cpu(), torch.gather(rows, 1, i.to(DEV)).cpu(), 'predict against _score_rows')
    hooks = m.combine_user_item_representations(m.get_user_representations(u), m.get_item_representations(torch.arange(R.N_ITEMS)))
    _assert_bits(hooks.cpu(), rows.cpu(), 'the evaluation hooks against _score_rows')
    m.save_model_to_path(str(tmp_path))
    other = Sm.RecVAE(device=DEV)
    other.load_model_from_path(str(tmp_path))
    assert (other.hidden, other.latent, other.gamma, other.beta, other.n_enc_epochs, other.seed) == (32, 8, 0.005, None, 3, 0)
    with pytest.raises(RuntimeError, match='attach'):
        other.predict(u, i)
    other.attach(train)
    _assert_bits(other._score_rows(u.to(DEV)).cpu(), rows.cpu(), 'a loaded model scores as the saved one')
    with np.load(tmp_path / 'model.npz') as f:
        assert set(R.PARAMS) <= set(f.files) and str(f['name']) == 'RecVAE' and f['fc_w1'].shape == (32, 40) and f['dec_w'].shape == (40, 8)
        broken = {k: f[k] for k in f.files}
    broken['ln_w3'] = broken['ln_w3'][:-1]
    np.savez(tmp_path / 'model.npz', **broken)
    with pytest.raises(ValueError, match='do not belong'):
        Sm.RecVAE(device=DEV).load_model_from_path(str(tmp_path))
    with pytest.raises(RuntimeError, match='fit'):
        Sm.RecVAE(device=DEV).predict(u, i)
    with pytest.raises(ValueError, match='0/1|other than 1'):
        Sm.RecVAE(device=DEV, n_epochs=0).fit(train * 2.0)


def test_registry_conf_and_the_constant_weight():
    Sm = S()
    assert Sm.ALGORITHMS['recvae'] is Sm.RecVAE
    conf = dict(hidden=12, latent=5, dropout=0.25, gamma=0.01, beta=0.3, lr=3e-3, batch_size=7, n_epochs=2, n_enc_epochs=2, n_dec_epochs=2,
                weight_decay=1e-4, seed=8)
    c = Sm.ALGORITHMS['recvae'].build_from_conf(conf, None)
    assert {k: getattr(c, k) for k in conf} == conf and c.name == 'RecVAE'
    with pytest.raises(ValueError, match='gamma and beta'):
        Sm.RecVAE(gamma=None, beta=None, device=DEV)
    train = R.planted_world(0)
    m = Sm.RecVAE(gamma=None, beta=0.2, device=DEV, n_epochs=0, **{k: v for k, v in CONF.items() if k != 'gamma'}).fit(train)
    users = torch.arange(5, device=DEV)
    assert torch.equal(m.kl_weight(users).cpu(), torch.full((5,), 0.2))
    g = prepared()
    counts = torch.from_numpy(np.diff(train.indptr)[:5].astype(np.float32))
    assert torch.equal(g.kl_weight(users).cpu(), counts * 0.005)
