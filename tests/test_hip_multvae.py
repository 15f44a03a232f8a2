"""Mult-VAE / Mult-DAE on the GPU (multvae.py, ``ops.MultinomialNLLFn`` over 'sbr_multinomial_nll_f32'): the autograd function and the
models against the float64 definitions of tests/multvae_ref.py, within 8 times the error the same formulas make in torch float32 on the
CPU (no floor); the value-dropout view; one Adam step; ``fit`` on the planted world against PopularItems; the evaluation routes, predict,
model.npz, deterministic mode and the registry."""
import functools
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import multvae_ref as R
from hip_testutil import DEV, S, U32, _assert_bits, call, stream

pytestmark = pytest.mark.gpu
ENTRY = 'sbr_multinomial_nll_f32'


def _mod(name):
    return import_module(S().ops.__name__.rsplit('.', 1)[0] + '.' + name)


def random_world(n_users, n_items, seed):
    rng = np.random.default_rng(seed)
    dense = (rng.random((n_users, n_items)) < 0.15).astype(np.float64)
    dense[1] = 0                                                       # a user without items
    dense[2] = 0
    dense[2, n_items - 1] = 1                                          # a user with one item: the normalised value is 1
    m = sp.csr_matrix(dense)
    m.sort_indices()
    return m, dense


def model_with(cls_name, train, hidden, latent, p, **kw):
    """the package's model with the parameters ``p`` of the float64 reference"""
    Sm = S()
    m = getattr(Sm, cls_name)(hidden=hidden, latent=latent, device=DEV, **kw)
    m.attach(train)
    net = _mod('multvae').AutoencoderWeights(train.shape[1], hidden, latent, m.code)
    with torch.no_grad():
        for k in R.PARAMS:
            getattr(net, k).copy_(p[k].detach().float())
    m.net = net.to(DEV)
    assert m.net.w_enc1.t().is_contiguous()
    return m


# ---- 1. the autograd function ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('inplace', [False, True])
@pytest.mark.parametrize('n_items', [30, 1027, 4100])
def test_autograd_function_against_float64(n_items, inplace):
    ops = S().ops
    train, dense = random_world(9, n_items, n_items)
    csr = _mod('features').DeviceCSR(train).to(DEV)
    z = np.random.default_rng(1).standard_normal((9, n_items)).astype(np.float32)
    loss64, _, d64 = R.nll64(z, dense, 1.0 / 9)
    eloss, _, ed = R.nll_bound(z, dense, np.float32(1.0 / 9))
    base = torch.from_numpy(z).to(DEV).requires_grad_()
    logits = base * 1.0                                                # a non-leaf: the function may write over it
    rows = torch.arange(9, device=DEV)
    loss = ops.MultinomialNLLFn.apply(csr, rows, logits, inplace)
    (3.0 * loss).backward()
    assert abs(float(loss.detach()) - loss64.mean()) <= eloss.mean() + 16 * U32 * np.abs(loss64).mean()
    err = np.abs(base.grad.cpu().double().numpy() - 3.0 * d64)
    assert (err <= 3.0 * ed + 4 * U32 * np.abs(3.0 * d64)).all(), f'worst {float((err - 3.0 * ed).max())}'
    if not inplace:
        assert torch.equal(logits.detach().cpu(), torch.from_numpy(z))
    unit = torch.from_numpy(z).to(DEV).requires_grad_()
    ops.MultinomialNLLFn.apply(csr, rows, unit * 1.0, inplace, True).backward()
    _assert_bits(unit.grad.cpu() * 3.0, base.grad.cpu(), 'unit_upstream hands the stored gradient on')
    with torch.no_grad():                                              # no gradient asked for: no gradient computed, the logits stay
        keep = torch.from_numpy(z).to(DEV)
        ops.MultinomialNLLFn.apply(csr, rows, keep, True)
        assert torch.equal(keep.cpu(), torch.from_numpy(z))


# ---- 2. the models against the float64 model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(40, 30, 8, 4), (64, 257, 64, 16)])
@pytest.mark.parametrize('cls_name', ['MultVAE', 'MultDAE'])
def test_models_against_float64(cls_name, shape):
    n_users, n_items, hidden, latent = shape
    variational = cls_name == 'MultVAE'
    train, dense = random_world(n_users, n_items, 5)
    p64 = R.init_params(n_items, hidden, latent, variational, 3)
    with torch.no_grad():
        for k in R.PARAMS:
            p64[k].mul_(4 if k.startswith('w') else 100)               # logits and biases of a size that matters
            p64[k].copy_(p64[k].float().double())                      # fp32-representable: every side starts from the same numbers
    p32 = {k: v.detach().float().requires_grad_() for k, v in p64.items()}
    x = torch.from_numpy(dense)
    eps = torch.randn(n_users, latent, generator=torch.Generator().manual_seed(1)).double()
    beta = 0.13
    out64 = R.forward(p64, x, variational, eps, None, 0.0, beta)
    out64[0].backward()
    out32 = R.forward(p32, x, variational, eps, None, 0.0, beta)
    out32[0].backward()
    m = model_with(cls_name, train, hidden, latent, p64)
    users = torch.arange(n_users, device=DEV)
    loss, nll, kl, logits = m.loss(users, beta, eps.float().to(DEV) if variational else None, dropout_seed=None, inplace=False)
    loss.backward()

    def check(name, got, ref64, ref32):
        tol = 8 * float((ref32.detach().double() - ref64.detach()).abs().max())
        err = float((got.detach().cpu().double() - ref64.detach()).abs().max())
        print(f'{cls_name} {shape} {name}: error {err:.3e}, 8 x float32-CPU error {tol:.3e}')
        assert err <= tol, f'{name}: {err} > {tol}'

    check('loss', loss, out64[0], out32[0])
    check('logits', logits, out64[3], out32[3])
    for k in R.PARAMS:
        check('grad ' + k, getattr(m.net, k).grad, p64[k].grad, p32[k].grad)
    # scoring: z = mu, no noise, no dropout
    with torch.no_grad():
        s64, s32 = R.forward(p64, x, variational)[3], R.forward(p32, x, variational)[3]
    check('score rows', m._score_rows(users), s64, s32)


# ---- 3. the value-dropout view ------------------------------------------------------------------------------------------------------------------
def test_dropout_view_is_dropout_of_the_value_vector():
    train, dense = random_world(40, 30, 2)
    m = S().MultDAE(hidden=8, latent=4, dropout=0.5, device=DEV)
    m.attach(train)
    base = m._input
    values = base.data.clone()
    want = torch.empty_like(values)
    call('sbr_dropout', values.data_ptr(), want.data_ptr(), values.numel(), 0.5, 12345, stream())
    view = m.dropped_input(12345)
    _assert_bits(view.data.cpu(), want.cpu(), 'the view\'s values')
    assert view.indptr.data_ptr() == base.indptr.data_ptr() and view.indices.data_ptr() == base.indices.data_ptr()
    assert 0 < int((want == 0).sum()) < want.numel() and torch.equal(base.data, values)
    fresh = _mod('features').DeviceCSR(sp.csr_matrix((want.cpu().numpy(), train.indices, train.indptr), shape=train.shape)).to(DEV)
    for a, b in zip(view.transposed(), fresh.transposed()):
        assert torch.equal(a, b), 'the transposed structure and values'
    users = torch.arange(40, device=DEV)
    assert torch.equal(view.dense_rows(users), fresh.dense_rows(users))
    again = m.dropped_input(777)
    assert again is view and not torch.equal(again.data, want)


# ---- 4. one Adam step -----------------------------------------------------------------------------------------------------------------------------
def test_one_adam_step_against_torch():
    train, _ = random_world(40, 30, 5)
    p = R.init_params(30, 8, 4, True, 2)
    m = model_with('MultVAE', train, 8, 4, p)
    opt = S().FusedOptimizer(m.net, 'adam', 1e-2, 0.)
    users = torch.arange(40, device=DEV)
    eps = torch.randn(40, 4, generator=torch.Generator().manual_seed(1)).to(DEV)
    m.loss(users, 0.1, eps, dropout_seed=3)[0].backward()
    opt._sync_grads()
    host = {k: getattr(m.net, k).detach().cpu().clone().requires_grad_() for k in R.PARAMS}
    for k in R.PARAMS:
        host[k].grad = getattr(m.net, k).grad.detach().cpu().clone()
    assert m.net.w_enc1.t().is_contiguous(), 'FlatParameters keeps the column-major layout'
    before = {k: getattr(m.net, k).detach().cpu().clone() for k in R.PARAMS}
    opt.step()
    torch.optim.Adam(list(host.values()), lr=1e-2).step()
    for k in R.PARAMS:
        got, want = getattr(m.net, k).detach().cpu().double(), host[k].detach().double()
        assert bool(((got - want).abs() <= 8 * U32 * (want.abs() + 1e-2)).all()), k
        assert not torch.equal(got.float(), before[k]), f'{k} did not move'


# ---- 5. fit on the planted world ---------------------------------------------------------------------------------------------------------------------
def eval_view(train, held):
    n_users, n_items = train.shape
    holdout = sp.csr_matrix((np.ones(held.size), (np.repeat(np.arange(n_users), held.shape[1]), held.reshape(-1))), shape=train.shape)
    return SimpleNamespace(n_users=n_users, n_items=n_items, items_in_split=np.arange(n_items), users_in_split=np.arange(n_users),
                           n_items_in_split=n_items, n_users_in_split=n_users, user_sampling_matrix=holdout, exclude_data=train.astype(bool),
                           user_features={}, item_features={})


def evaluate(alg, view, **kw):
    Sm = S()
    ev = Sm.FullEvaluator(config=Sm.evaluation._Cfg(top_k=(10,)), dataset=view)
    return Sm.evaluate_recommender_algorithm(alg, type('L', (), {'dataset': view, 'batch_size': 64})(), ev, DEV, **kw)


@functools.lru_cache(maxsize=None)
def fitted(cls_name, seed):
    train, held = R.planted_world(seed)
    return getattr(S(), cls_name)(seed=seed, device=DEV, **R.SETTINGS).fit(train), train, held


@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('cls_name', ['MultVAE', 'MultDAE'])
def test_fit_beats_popularity_twice_over(cls_name, seed):
    Sm = S()
    m, train, held = fitted(cls_name, seed)
    view = eval_view(train, held)
    got = evaluate(m, view)['ndcg@10']
    pop = evaluate(Sm.PopularItems.build_from_conf({}, SimpleNamespace(user_sampling_matrix=train)), view)['ndcg@10']
    print(f'{cls_name} seed {seed}: NDCG@10 {got:.4f}, PopularItems {pop:.4f}, last epoch loss {m.epoch_losses[-1]:.4f}')
    assert len(m.epoch_losses) == R.SETTINGS['n_epochs'] and m.epoch_losses[-1] < m.epoch_losses[0]
    assert got >= 2 * pop


def test_scorers_predict_and_persistence(tmp_path):
    Sm = S()
    m, train, held = fitted('MultVAE', 0)
    view = eval_view(train, held)
    base = evaluate(m, view, scorer='fp32')
    fused = evaluate(m, view, scorer='fp32_fused')
    assert set(fused) == set(base) and all(np.array_equal(fused[k], base[k]) for k in base), 'the item side is a tuple: every scorer takes the fp32 route'
    u = torch.tensor([0, 5, 239, 17])
    i = torch.tensor([[0, 95, 3], [1, 2, 3], [50, 51, 52], [7, 7, 8]])
    rows = m.combine_user_item_representations(m.get_user_representations(u), m.get_item_representations(torch.arange(96)))
    _assert_bits(m.predict(u, i).cpu(), torch.gather(rows, 1, i.to(DEV)).cpu(), 'predict against the evaluation\'s score rows')
    m.save_model_to_path(str(tmp_path))
    other = Sm.MultVAE(device=DEV)
    other.load_model_from_path(str(tmp_path))
    assert (other.hidden, other.latent, other.seed) == (m.hidden, m.latent, m.seed)
    with pytest.raises(RuntimeError, match='attach'):
        other.predict(u, i)
    other.attach(train)
    _assert_bits(other.predict(u, i).cpu(), m.predict(u, i).cpu(), 'a loaded model scores as the saved one')
    with np.load(tmp_path / 'model.npz') as f:
        assert set(R.PARAMS) <= set(f.files) and str(f['name']) == 'MultVAE' and f['w_enc1'].shape == (32, 96)
    with pytest.raises(ValueError, match='MultVAE'):
        Sm.MultDAE(device=DEV).load_model_from_path(str(tmp_path))
    Sm.EASE(5, device=DEV).fit(train).save_model_to_path(str(tmp_path))
    with pytest.raises(ValueError, match='not a model of this package'):
        Sm.MultVAE(device=DEV).load_model_from_path(str(tmp_path))
    with pytest.raises(RuntimeError, match='fit'):
        Sm.MultVAE(device=DEV).predict(u, i)


def test_deterministic_mode():
    Sm = S()
    train, _ = R.planted_world(0)
    conf = {**R.SETTINGS, 'n_epochs': 3}
    prev = Sm.ops.set_deterministic(True)
    try:
        for cls in (Sm.MultVAE, Sm.MultDAE):
            a, b = (cls(seed=4, device=DEV, **conf).fit(train) for _ in range(2))
            for k in R.PARAMS:
                assert torch.equal(getattr(a.net, k), getattr(b.net, k)), f'{cls.__name__}: {k} differs between two fits'
            assert a.epoch_losses == b.epoch_losses
        with pytest.raises(Sm.SibrarHipError, match='no deterministic form'):
            Sm.MultVAE(seed=4, device=DEV, **{**conf, 'hidden': 600}).fit(train)
    finally:
        Sm.ops.set_deterministic(prev)


def test_registry_and_conf():
    Sm = S()
    assert Sm.ALGORITHMS['multvae'] is Sm.MultVAE and Sm.ALGORITHMS['multdae'] is Sm.MultDAE
    assert issubclass(Sm.MultVAE, Sm.ResidentMatrixAlgorithm) and issubclass(Sm.MultDAE, Sm.ResidentMatrixAlgorithm)
    d = Sm.ALGORITHMS['multvae'].build_from_conf({}, None)
    assert (d.hidden, d.latent, d.dropout, d.lr, d.batch_size, d.anneal_cap, d.total_anneal_steps, d.weight_decay, d.seed) == \
        (600, 200, 0.5, 1e-3, 500, 0.2, 200000, 0., 0)
    conf = dict(hidden=12, latent=5, dropout=0.25, lr=3e-3, batch_size=7, anneal_cap=0.5, total_anneal_steps=9, n_epochs=2, weight_decay=1e-4, seed=8)
    c = Sm.ALGORITHMS['multdae'].build_from_conf(conf, None)
    assert {k: getattr(c, k) for k in conf} == conf and c.name == 'MultDAE' and c.code == 5 and d.code == 400
