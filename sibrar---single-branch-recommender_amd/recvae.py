"""RecVAE (Shenbin, Alekseev, Tutubalina, Malykh, Nikolenko, WSDM 2020; registry name ``recvae``): the variational autoencoder over a
user's interaction row with a deeper encoder, a prior that is a mixture with the previous epoch's posterior, a KL weight proportional to
the user's interaction count, and alternating encoder / decoder updates. The reference has no autoencoder of this kind; this is not a
port. The definitions below follow the authors' published code as remembered: that code could not be consulted while this was written,
so they are unchecked against it. tests/recvae_ref.py restates them in float64.

Encoder: ``x`` is the user's L2-normalised 0/1 row, with input dropout in training. ``h1 = LN(swish(fc1 x))``, ``hk = LN(swish(fck h(k-1) +
h1 + .. + h(k-1)))`` for k = 2..5 (LayerNorm with eps 0.1), ``mu = fc_mu h5``, ``logvar = fc_logvar h5``. Decoder: one linear layer.
Prior: ``log p(z | x) = logsumexp(log(3/20) + log N(z; 0, 0), log(3/4) + log N(z; mu_old(x), logvar_old(x)), log(1/10) + log N(z; 0, 10))``
with the frozen "old" encoder, run on ``x`` without dropout. Loss: ``nll + mean_b weight_b sum_j (log N(z; mu, logvar) - log p(z | x))`` with
``z = mu + eps exp(logvar / 2)``, ``weight_b = gamma n_b`` (``n_b`` the user's interaction count), or the constant ``beta`` when ``gamma`` is
None or 0.

Nothing is densified. The input layer is ``ops.SparseLinearActFn`` on ``DeviceCSR(m, l2_normalize_rows=True)`` with value-level dropout
(``ops.DropoutFn`` over the value view), as in multvae.py. Each of the five layer tails is one launch of ``ops.SwishLayerNormFn``, which
also carries the running sum ``h1 + .. + hk``; the reparameterisation and the KL term are one launch of ``ops.CompositePriorKLFn``; the
likelihood is ``ops.MultinomialNLLFn``. Encoder and decoder are two modules with a ``FusedOptimizer('adam')`` each. The old encoder is a
set of plain tensors that own their storage (``update_prior`` clones: the encoder's parameters live in the optimizer's flat buffer, and a
view of that would follow every step).

One epoch of ``fit``: ``n_enc_epochs`` passes over a fresh seeded permutation of the users that have an interaction update the encoder
(input dropout ``dropout``), ``update_prior()``, then ``n_dec_epochs`` passes update the decoder (no dropout, the encoder under
``no_grad``). One synchronisation per epoch, for the logged loss: the mean loss of the epoch's last pass.

Scoring: ``_score_rows(u)`` is ``decoder(mu)`` without dropout or noise. The decoder's bias makes the item side of the evaluation hooks a
tuple, so every ``scorer`` takes the ``fp32`` route. Deterministic mode: two fits from one seed give the same bits where ``hidden`` is a
multiple of 4 and at most 512 (``sbr_csr_project_bwd_gather``) and the widths are ones ``sbr_colsum`` takes in its fixed-slot form; the
two kernels of this model have no other form.
"""
from __future__ import annotations

import logging
import math
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp
import torch
from torch import nn

from . import ops
from .features import DeviceCSR
from .matrix_models import ResidentMatrixAlgorithm
from .optim import FusedOptimizer

N_LAYERS = 5
LN_EPS = 0.1
ENCODER_PARAMS = tuple(f'{kind}{k}' for k in range(1, N_LAYERS + 1) for kind in ('fc_w', 'fc_b', 'ln_w', 'ln_b')) + \
    ('mu_w', 'mu_b', 'logvar_w', 'logvar_b')
DECODER_PARAMS = ('dec_w', 'dec_b')
PARAMS = ENCODER_PARAMS + DECODER_PARAMS
HYPER = ('hidden', 'latent', 'dropout', 'gamma', 'beta', 'lr', 'batch_size', 'n_epochs', 'n_enc_epochs', 'n_dec_epochs', 'weight_decay', 'seed')


def encoder_shapes(n_items: int, hidden: int, latent: int) -> dict:
    shapes = {}
    for k in range(1, N_LAYERS + 1):
        shapes[f'fc_w{k}'], shapes[f'fc_b{k}'] = (hidden, n_items if k == 1 else hidden), (hidden,)
        shapes[f'ln_w{k}'] = shapes[f'ln_b{k}'] = (hidden,)
    shapes.update(mu_w=(latent, hidden), mu_b=(latent,), logvar_w=(latent, hidden), logvar_b=(latent,))
    return shapes


class RecVAEEncoder(nn.Module):
    """``fc_w1`` [hidden, I] stored column-major (``SparseLinearActFn``'s layout), ``fc_w2..5`` [hidden, hidden], the LayerNorms'
    ``ln_w`` = 1 and ``ln_b`` = 0, and the two heads [latent, hidden]. Weights are Xavier-normal, biases normal with std 0.001, drawn on
    the host from ``generator`` in the order of ``ENCODER_PARAMS``."""

    def __init__(self, n_items: int, hidden: int, latent: int, generator: torch.Generator):
        super().__init__()
        for name, shape in encoder_shapes(n_items, hidden, latent).items():
            if name.startswith('ln_'):
                t = torch.ones(shape) if name.startswith('ln_w') else torch.zeros(shape)
            elif len(shape) == 2:
                t = torch.randn(*shape, generator=generator) * math.sqrt(2.0 / (shape[0] + shape[1]))
                if name == 'fc_w1':
                    t = t.t().contiguous().t()
            else:
                t = torch.randn(*shape, generator=generator) * 0.001
            setattr(self, name, nn.Parameter(t))


class RecVAEDecoder(nn.Module):
    """``dec_w`` [I, latent] Xavier-normal and ``dec_b`` [I] normal with std 0.001, drawn after the encoder's from the same generator"""

    def __init__(self, n_items: int, latent: int, generator: torch.Generator):
        super().__init__()
        self.dec_w = nn.Parameter(torch.randn(n_items, latent, generator=generator) * math.sqrt(2.0 / (n_items + latent)))
        self.dec_b = nn.Parameter(torch.randn(n_items, generator=generator) * 0.001)


def encode(p, csr: DeviceCSR, u: torch.Tensor):
    """-> (mu, logvar) [B, latent] of the rows ``u`` of ``csr``; ``p``: anything with the encoder's arrays as attributes"""
    a = ops.SparseLinearActFn.apply(csr, u, p.fc_w1, p.fc_b1, 0)
    h, r = ops.SwishLayerNormFn.apply(a, None, p.ln_w1, p.ln_b1, LN_EPS, True)
    for k in range(2, N_LAYERS + 1):
        a = ops.LinearActFn.apply(h, getattr(p, f'fc_w{k}'), getattr(p, f'fc_b{k}'), 0)
        h, r = ops.SwishLayerNormFn.apply(a, r, getattr(p, f'ln_w{k}'), getattr(p, f'ln_b{k}'), LN_EPS, k < N_LAYERS)
    return ops.LinearActFn.apply(h, p.mu_w, p.mu_b, 0), ops.LinearActFn.apply(h, p.logvar_w, p.logvar_b, 0)


class RecVAE(ResidentMatrixAlgorithm):
    """``kwargs``: ``device``. ``fit(matrix)`` trains; ``encoder`` and ``decoder`` hold the weights afterwards (None: not fitted)."""
    KEY, WHAT = 'dec_w', 'weights'
    STORES = 'the encoder\'s and the decoder\'s weight arrays'
    BINARY_ONLY = 'RecVAE: the multinomial likelihood takes the 0/1 rows as its targets'

    def __init__(self, hidden: int = 600, latent: int = 200, dropout: float = 0.5, gamma: float = 0.005, beta: float = None, lr: float = 5e-4,
                 batch_size: int = 500, n_epochs: int = 50, n_enc_epochs: int = 3, n_dec_epochs: int = 1, weight_decay: float = 0.,
                 seed: int = 0, **kwargs):
        super().__init__(kwargs.get('device'))
        if hidden < 1 or latent < 1 or batch_size < 1 or n_epochs < 0 or n_enc_epochs < 0 or n_dec_epochs < 0:
            raise ValueError(f'hidden={hidden}, latent={latent}, batch_size={batch_size} must be positive and n_epochs={n_epochs}, '
                             f'n_enc_epochs={n_enc_epochs}, n_dec_epochs={n_dec_epochs} not negative')
        if not 0 <= dropout < 1:
            raise ValueError(f'dropout={dropout!r} outside [0, 1)')
        if gamma is None and beta is None:
            raise ValueError('RecVAE: gamma and beta are both unset: the KL term needs its weight (gamma * interactions, or the constant beta)')
        self.hidden, self.latent, self.dropout, self.lr, self.batch_size = int(hidden), int(latent), float(dropout), float(lr), int(batch_size)
        self.gamma, self.beta = None if gamma is None else float(gamma), None if beta is None else float(beta)
        if not self.gamma and self.beta is None:
            raise ValueError('RecVAE: gamma is 0 and beta is unset: the KL term needs its weight')
        self.n_epochs, self.n_enc_epochs, self.n_dec_epochs = int(n_epochs), int(n_enc_epochs), int(n_dec_epochs)
        self.weight_decay, self.seed = float(weight_decay), int(seed)
        self.encoder = self.decoder = self.old = None
        self._input = self._dropped = self._weight = None
        self.epoch_losses = []
        self.name = 'RecVAE'
        logging.info(f'Built {self.name} module \n- hidden: {self.hidden} \n- latent: {self.latent} \n- dropout: {self.dropout} \n- gamma: {self.gamma} ')

    @classmethod
    def build_from_conf(cls, conf: dict, dataset=None):
        return cls(**{k: conf[k] for k in HYPER if k in conf})

    @property
    def dec_w(self):
        return None if self.decoder is None else self.decoder.dec_w

    # ---- residency ---------------------------------------------------------------------------------------------------------------
    def _resident(self, m: sp.csr_matrix) -> DeviceCSR:
        self._input = DeviceCSR(m, l2_normalize_rows=True).to(self.device)
        self._dropped = self._weight = None
        return DeviceCSR(m)

    def to(self, device):
        super().to(device)
        if self._input is not None:
            self._input, self._dropped, self._weight = self._input.to(self.device), None, None
        if self.encoder is not None:
            self.encoder, self.decoder = self.encoder.to(self.device), self.decoder.to(self.device)
        if self.old is not None:
            self.old = SimpleNamespace(**{k: v.to(self.device) for k, v in vars(self.old).items()})
        return self

    def _build(self, n_items: int):
        g = torch.Generator().manual_seed(self.seed)
        self.encoder = RecVAEEncoder(n_items, self.hidden, self.latent, g).to(self.device)
        self.decoder = RecVAEDecoder(n_items, self.latent, g).to(self.device)
        self.update_prior()

    # ---- the network ---------------------------------------------------------------------------------------------------------------
    def update_prior(self):
        """the old encoder becomes a copy of the encoder: clones that own their storage, not views of the optimizer's flat buffer"""
        self.old = SimpleNamespace(**{k: getattr(self.encoder, k).detach().clone(memory_format=torch.preserve_format) for k in ENCODER_PARAMS})

    def decode(self, z: torch.Tensor) -> torch.Tensor:
        return ops.LinearActFn.apply(z, self.decoder.dec_w, self.decoder.dec_b, 0)

    def dropped_input(self, seed: int) -> DeviceCSR:
        """the normalised rows with ``sbr_dropout(p = dropout, seed)`` applied to their stored values"""
        if self._dropped is None:
            self._dropped = self._input.value_view()
            self._kept_values = self._dropped.data
        return self._dropped.replace_values(ops.DropoutFn.apply(self._kept_values, self.dropout, int(seed)))

    def kl_weight(self, u: torch.Tensor) -> torch.Tensor:
        """``gamma * n_b`` of the users ``u``, from the resident matrix's ``indptr``; the constant ``beta`` when ``gamma`` is None or 0"""
        if self._weight is None:
            counts = (self._matrix.indptr[1:] - self._matrix.indptr[:-1]).to(torch.float32)
            self._weight = counts * self.gamma if self.gamma else torch.full_like(counts, self.beta)
        return self._weight[u]

    def loss(self, u: torch.Tensor, eps: torch.Tensor, dropout_seed: int = None, inplace: bool = True, encoder_grad: bool = True):
        """-> (loss, nll, kld, logits) of the batch of users ``u`` (int64 [B] on the device) with the noise ``eps`` [B, latent];
        ``dropout_seed`` None: no input dropout. With ``inplace`` the logits are overwritten by their gradient when they need one.
        ``encoder_grad=False``: the encoder runs under ``no_grad`` (a decoder pass)."""
        csr = self.dropped_input(dropout_seed) if dropout_seed is not None and self.dropout > 0 else self._input
        with torch.set_grad_enabled(encoder_grad and torch.is_grad_enabled()):
            mu, logvar = encode(self.encoder, csr, u)
        with torch.no_grad():
            mu_old, logvar_old = encode(self.old, self._input, u)
        z, kld = ops.CompositePriorKLFn.apply(mu, logvar, eps, mu_old, logvar_old, self.kl_weight(u))
        logits = self.decode(z)
        nll = ops.MultinomialNLLFn.apply(self._matrix, u, logits, inplace, True)
        return nll + kld, nll, kld, logits

    # ---- training ------------------------------------------------------------------------------------------------------------------
    def fit(self, matrix: sp.spmatrix, **kwargs):
        """:param matrix: user x item sparse matrix, 0/1"""
        self.attach(matrix)
        self.encoder = self.decoder = self.old = None
        self._build(self.n_items)
        self._opt_enc = FusedOptimizer(self.encoder, 'adam', self.lr, self.weight_decay)
        self._opt_dec = FusedOptimizer(self.decoder, 'adam', self.lr, self.weight_decay)
        self.update_prior()
        self._gen = torch.Generator(device=self.device).manual_seed(self.seed)
        counts = self._matrix.indptr[1:] - self._matrix.indptr[:-1]
        self._active = torch.nonzero(counts > 0).reshape(-1)
        self._step, self.epoch_losses = 0, []
        for epoch in range(self.n_epochs):
            self.train_epoch()
            logging.info(f'{self.name}: epoch {epoch} loss {self.epoch_losses[-1]:.6f}')
        return self

    def train_pass(self, part: str) -> torch.Tensor:
        """One pass over a fresh permutation of the users that have an interaction, updating the encoder (``part='encoder'``, input
        dropout) or the decoder (``'decoder'``, no dropout, the encoder without gradients) -> the sum of the batch losses times the
        batch sizes, on the device (no synchronisation)."""
        enc = part == 'encoder'
        if not enc and part != 'decoder':
            raise ValueError(f'train_pass: part={part!r} is neither encoder nor decoder')
        opt, gen = (self._opt_enc if enc else self._opt_dec), self._gen
        for p in self.decoder.parameters():
            p.requires_grad_(not enc)
        order = self._active[torch.randperm(self._active.numel(), generator=gen, device=self.device)]
        total = torch.zeros((), device=self.device)
        try:
            for lo in range(0, order.numel(), self.batch_size):
                u = order[lo:lo + self.batch_size].contiguous()
                eps = torch.randn(u.numel(), self.latent, generator=gen, device=self.device)
                loss = self.loss(u, eps, dropout_seed=(self.seed << 32) + self._step if enc else None, encoder_grad=enc)[0]
                loss.backward()
                opt.step()
                opt.zero_grad()
                total += loss.detach() * u.numel()
                self._step += 1
        finally:
            for p in self.decoder.parameters():
                p.requires_grad_(True)
        return total

    def train_epoch(self) -> float:
        """``n_enc_epochs`` encoder passes, ``update_prior()``, ``n_dec_epochs`` decoder passes (after ``fit`` has set the training state
        up, also with ``n_epochs=0``) -> the mean loss of the epoch's last pass, also appended to ``epoch_losses``: the epoch's one
        synchronisation."""
        last = torch.zeros((), device=self.device)
        for _ in range(self.n_enc_epochs):
            last = self.train_pass('encoder')
        self.update_prior()
        for _ in range(self.n_dec_epochs):
            last = self.train_pass('decoder')
        self.epoch_losses.append(float(last) / max(self._active.numel(), 1))
        return self.epoch_losses[-1]

    # ---- scoring -------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _score_rows(self, u: torch.Tensor) -> torch.Tensor:
        if self.encoder.fc_w1.shape[1] != self.n_items:
            raise ValueError(f'{self.name}: weights for {self.encoder.fc_w1.shape[1]} items do not fit the {self.n_items} items of the matrix')
        return self.decode(encode(self.encoder, self._input, u.long().contiguous())[0])

    # ---- persistence ---------------------------------------------------------------------------------------------------------------
    def _arrays(self) -> dict:
        return {**{k: getattr(self.encoder, k) for k in ENCODER_PARAMS}, **{k: getattr(self.decoder, k) for k in DECODER_PARAMS}}

    def _npz_fields(self) -> dict:
        hyper = {h: np.array(np.nan if getattr(self, h) is None else getattr(self, h)) for h in HYPER}       # None (gamma, beta) is stored as NaN
        return {**{k: v.detach().cpu().numpy() for k, v in self._arrays().items()}, **hyper}

    def _read_npz(self, f):
        missing = [k for k in PARAMS + HYPER if k not in f.files]
        if missing:
            raise ValueError(f'model.npz: no {missing}')
        hyper = {h: f[h].item() for h in HYPER}
        w = {k: f[k] for k in PARAMS}
        hidden, latent = int(hyper['hidden']), int(hyper['latent'])
        n_items = w['fc_w1'].shape[1] if w['fc_w1'].ndim == 2 else -1
        want = {**encoder_shapes(n_items, hidden, latent), 'dec_w': (n_items, latent), 'dec_b': (n_items,)}
        bad = {k: w[k].shape for k in PARAMS if tuple(w[k].shape) != want[k]}
        if bad:
            raise ValueError(f'model.npz: arrays of shapes {bad} do not belong to a {self.name} with hidden={hidden}, latent={latent}')
        g = torch.Generator().manual_seed(0)
        encoder, decoder = RecVAEEncoder(n_items, hidden, latent, g), RecVAEDecoder(n_items, latent, g)
        with torch.no_grad():
            for k in PARAMS:
                getattr(encoder if k in ENCODER_PARAMS else decoder, k).copy_(torch.from_numpy(w[k].astype(np.float32)))
        for h in HYPER:
            v = hyper[h]
            if h in ('gamma', 'beta'):
                setattr(self, h, None if math.isnan(v) else float(v))
            else:
                setattr(self, h, type(getattr(self, h))(v))
        self.encoder, self.decoder = encoder.to(self.device), decoder.to(self.device)
        self._weight = None
        self.update_prior()
