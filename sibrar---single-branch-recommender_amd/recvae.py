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

from types import SimpleNamespace

import torch

from . import ops
from .features import DeviceCSR
from .row_autoencoder import RowAutoencoder

N_LAYERS = 5
LN_EPS = 0.1
ENCODER_PARAMS = tuple(f'{kind}{k}' for k in range(1, N_LAYERS + 1) for kind in ('fc_w', 'fc_b', 'ln_w', 'ln_b')) + \
    ('mu_w', 'mu_b', 'logvar_w', 'logvar_b')
DECODER_PARAMS = ('dec_w', 'dec_b')
PARAMS = ENCODER_PARAMS + DECODER_PARAMS


def encode(p, csr: DeviceCSR, u: torch.Tensor):
    """-> (mu, logvar) [B, latent] of the rows ``u`` of ``csr``; ``p``: anything with the encoder's arrays as attributes"""
    a = ops.SparseLinearActFn.apply(csr, u, p.fc_w1, p.fc_b1, 0)
    h, r = ops.SwishLayerNormFn.apply(a, None, p.ln_w1, p.ln_b1, LN_EPS, True)
    for k in range(2, N_LAYERS + 1):
        a = ops.LinearActFn.apply(h, getattr(p, f'fc_w{k}'), getattr(p, f'fc_b{k}'), 0)
        h, r = ops.SwishLayerNormFn.apply(a, r, getattr(p, f'ln_w{k}'), getattr(p, f'ln_b{k}'), LN_EPS, k < N_LAYERS)
    return ops.LinearActFn.apply(h, p.mu_w, p.mu_b, 0), ops.LinearActFn.apply(h, p.logvar_w, p.logvar_b, 0)


class RecVAE(RowAutoencoder):
    """``kwargs``: ``device``. ``fit(matrix)`` trains; ``encoder`` and ``decoder`` hold the weights afterwards (None: not fitted)."""
    KEY, INPUT = 'dec_w', 'fc_w1'
    STORES = 'the encoder\'s and the decoder\'s weight arrays'
    BINARY_ONLY = 'RecVAE: the multinomial likelihood takes the 0/1 rows as its targets'
    HYPER = ('hidden', 'latent', 'dropout', 'gamma', 'beta', 'lr', 'batch_size', 'n_epochs', 'n_enc_epochs', 'n_dec_epochs', 'weight_decay', 'seed')
    OPTIONAL = ('gamma', 'beta')
    PARTS = {'encoder': ENCODER_PARAMS, 'decoder': DECODER_PARAMS}
    CONSTANTS = {f'ln_{kind}{k}': value for k in range(1, N_LAYERS + 1) for kind, value in (('w', 1.), ('b', 0.))}       # the LayerNorms' start

    def __init__(self, hidden: int = 600, latent: int = 200, dropout: float = 0.5, gamma: float = 0.005, beta: float = None, lr: float = 5e-4,
                 batch_size: int = 500, n_epochs: int = 50, n_enc_epochs: int = 3, n_dec_epochs: int = 1, weight_decay: float = 0.,
                 seed: int = 0, **kwargs):
        super().__init__(hidden, latent, dropout, lr, batch_size, n_epochs, weight_decay, seed, kwargs.get('device'))
        if n_enc_epochs < 0 or n_dec_epochs < 0:
            raise ValueError(f'n_enc_epochs={n_enc_epochs}, n_dec_epochs={n_dec_epochs} must not be negative')
        if gamma is None and beta is None:
            raise ValueError('RecVAE: gamma and beta are both unset: the KL term needs its weight (gamma * interactions, or the constant beta)')
        self.gamma, self.beta = None if gamma is None else float(gamma), None if beta is None else float(beta)
        if not self.gamma and self.beta is None:
            raise ValueError('RecVAE: gamma is 0 and beta is unset: the KL term needs its weight')
        self.n_enc_epochs, self.n_dec_epochs = int(n_enc_epochs), int(n_dec_epochs)
        self.old = None

    @classmethod
    def shapes(cls, n_items: int, hidden: int, latent: int) -> dict:
        """the encoder's arrays in the order of ``ENCODER_PARAMS``: ``fc_w1`` [hidden, I] stored column-major (``SparseLinearActFn``'s
        layout), ``fc_w2..5`` [hidden, hidden], the LayerNorms' ``ln_w`` = 1 and ``ln_b`` = 0, and the two heads [latent, hidden]; then the
        decoder's ``dec_w`` [I, latent] and ``dec_b`` [I], drawn after the encoder's from the same generator"""
        shapes = {}
        for k in range(1, N_LAYERS + 1):
            shapes[f'fc_w{k}'], shapes[f'fc_b{k}'] = (hidden, n_items if k == 1 else hidden), (hidden,)
            shapes[f'ln_w{k}'] = shapes[f'ln_b{k}'] = (hidden,)
        shapes.update(mu_w=(latent, hidden), mu_b=(latent,), logvar_w=(latent, hidden), logvar_b=(latent,), dec_w=(n_items, latent), dec_b=(n_items,))
        return shapes

    @property
    def dec_w(self):
        return None if self.decoder is None else self.decoder.dec_w

    @property
    def _opt_enc(self):
        return self._opts['encoder']

    # ---- residency ---------------------------------------------------------------------------------------------------------------
    def _forget_views(self):
        super()._forget_views()
        self._weight = None                    # kl_weight's per-user table

    def to(self, device):
        super().to(device)
        if self.old is not None:
            self.old = SimpleNamespace(**{k: v.to(self.device) for k, v in vars(self.old).items()})
        return self

    def _set_weights(self, tensors: dict):
        super()._set_weights(tensors)
        self._weight = None
        self.update_prior()

    # ---- the network ---------------------------------------------------------------------------------------------------------------
    def update_prior(self):
        """the old encoder becomes a copy of the encoder: clones that own their storage, not views of the optimizer's flat buffer"""
        self.old = SimpleNamespace(**{k: getattr(self.encoder, k).detach().clone(memory_format=torch.preserve_format) for k in ENCODER_PARAMS})

    def decode(self, z: torch.Tensor) -> torch.Tensor:
        return ops.LinearActFn.apply(z, self.decoder.dec_w, self.decoder.dec_b, 0)

    def _network(self, u: torch.Tensor) -> torch.Tensor:
        return self.decode(encode(self.encoder, self._input, u)[0])

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
        csr = self._rows_in(dropout_seed)
        with torch.set_grad_enabled(encoder_grad and torch.is_grad_enabled()):
            mu, logvar = encode(self.encoder, csr, u)
        with torch.no_grad():
            mu_old, logvar_old = encode(self.old, self._input, u)
        z, kld = ops.CompositePriorKLFn.apply(mu, logvar, eps, mu_old, logvar_old, self.kl_weight(u))
        logits = self.decode(z)
        nll = ops.MultinomialNLLFn.apply(self._matrix, u, logits, inplace, True)
        return nll + kld, nll, kld, logits

    # ---- training ------------------------------------------------------------------------------------------------------------------
    def _batch_loss(self, part: str, u: torch.Tensor, dropout_seed: int) -> torch.Tensor:
        enc = part == 'encoder'
        eps = torch.randn(u.numel(), self.latent, generator=self._gen, device=self.device)
        return self.loss(u, eps, dropout_seed if enc else None, encoder_grad=enc)[0]

    def train_pass(self, part: str) -> torch.Tensor:
        """A pass that updates the encoder (``part='encoder'``, input dropout) or the decoder (``'decoder'``, no dropout, the encoder
        without gradients)."""
        if part not in self.PARTS:
            raise ValueError(f'train_pass: part={part!r} is neither encoder nor decoder')
        for p in self.decoder.parameters():
            p.requires_grad_(part == 'decoder')
        try:
            return super().train_pass(part)
        finally:
            for p in self.decoder.parameters():
                p.requires_grad_(True)

    def _epoch(self) -> torch.Tensor:
        """``n_enc_epochs`` encoder passes, ``update_prior()``, ``n_dec_epochs`` decoder passes"""
        last = torch.zeros((), device=self.device)
        for _ in range(self.n_enc_epochs):
            last = self.train_pass('encoder')
        self.update_prior()
        for _ in range(self.n_dec_epochs):
            last = self.train_pass('decoder')
        return last
