"""Mult-VAE and Mult-DAE (Liang, Krishnan, Hoffman, Jebara, WWW 2018; registry names ``multvae`` and ``multdae``): autoencoders over a
user's interaction row with a multinomial likelihood over the whole catalogue. The reference has no autoencoder of this kind; these are
not ports.

The network is ``I -> hidden -> latent -> hidden -> I`` with tanh between the layers and none on the output. Mult-VAE's encoder ends in
``2 * latent`` values (mu, logvar), without an activation; the code is ``z = mu + eps * exp(0.5 * logvar)`` in training and ``mu`` for
scoring, and ``beta * KL`` with ``KL = mean_b 0.5 * sum(-logvar + exp(logvar) + mu^2 - 1)`` joins the loss, ``beta`` annealed linearly from 0
to ``anneal_cap`` over ``total_anneal_steps`` optimizer steps. Mult-DAE's encoder ends in ``latent`` values with a tanh; no sampling, no KL.

Nothing is densified. The input is the user's L2-normalised row (``DeviceCSR(m, l2_normalize_rows=True)``) into ``ops.SparseLinearActFn``
(its weight column-major); input dropout acts on the stored values of the rows (``sbr_dropout`` over the value vector through
``DeviceCSR.value_view``, a fresh seed per step), which is the paper's dropout of the dense row, because a zero stays a zero. The other
layers are ``ops.LinearActFn``. The loss is ``ops.MultinomialNLLFn`` (``sbr_multinomial_nll_f32``) against the resident 0/1 matrix: one
launch computes the loss and turns the logit matrix into its own gradient. The KL term and the reparameterisation are torch ops on
[B, 2 * latent]. ``fit`` trains with ``FusedOptimizer('adam')`` over a seeded permutation of the users that have an interaction, and
synchronises once per epoch, for the logged loss.

Scoring: ``_score_rows(u)`` is the decoder's output for the code ``mu`` (Mult-DAE: its code), without dropout or noise. The output bias
makes a score more than a dot product, so the item side of the evaluation hooks stays a tuple and every evaluation takes the ``fp32``
route (dense score rows, mask, top-k), whatever ``scorer`` asks for.

Deterministic mode: two fits from one seed give the same bits where every entry on the path has a fixed-order form, that is ``hidden`` a
multiple of 4 and at most 512 (``sbr_csr_project_bwd_gather``) and widths ``sbr_colsum`` takes in its fixed-slot form; outside them the
library's refusals surface unchanged.
"""
from __future__ import annotations

import torch

from . import ops
from .features import DeviceCSR
from .row_autoencoder import RowAutoencoder, Weights, init_weights

TANH = ops.ACT_CODES['tanh']
PARAMS = ('w_enc1', 'b_enc1', 'w_enc2', 'b_enc2', 'w_dec1', 'b_dec1', 'w_dec2', 'b_dec2')


def shapes(n_items: int, hidden: int, latent: int, code: int) -> dict:
    """The eight parameters: ``w_enc1`` [hidden, I] stored column-major (``SparseLinearActFn``'s layout), ``w_enc2`` [code, hidden] with
    code = 2 * latent (Mult-VAE) or latent (Mult-DAE), ``w_dec1`` [hidden, latent], ``w_dec2`` [I, hidden], and their biases."""
    return {'w_enc1': (hidden, n_items), 'b_enc1': (hidden,), 'w_enc2': (code, hidden), 'b_enc2': (code,), 'w_dec1': (hidden, latent),
            'b_dec1': (hidden,), 'w_dec2': (n_items, hidden), 'b_dec2': (n_items,)}


class AutoencoderWeights(Weights):
    """``shapes`` as a module, drawn on the host from ``seed`` (``init_weights``)"""

    def __init__(self, n_items: int, hidden: int, latent: int, code: int, seed: int = 0):
        super().__init__(init_weights(shapes(n_items, hidden, latent, code), torch.Generator().manual_seed(int(seed)), ('w_enc1',)))


class MultDAE(RowAutoencoder):
    """``kwargs``: ``device``. ``fit(matrix)`` trains; ``net`` holds the weights afterwards (None: not fitted)."""
    KEY = INPUT = 'w_enc1'
    STORES = 'the autoencoder\'s eight weight arrays'
    BINARY_ONLY = 'MultDAE: the multinomial likelihood takes the 0/1 rows as its targets'
    HYPER = ('hidden', 'latent', 'dropout', 'lr', 'batch_size', 'anneal_cap', 'total_anneal_steps', 'n_epochs', 'weight_decay', 'seed')
    PARTS = {'net': PARAMS}
    VARIATIONAL = False

    def __init__(self, hidden: int = 600, latent: int = 200, dropout: float = 0.5, lr: float = 1e-3, batch_size: int = 500,
                 anneal_cap: float = 0.2, total_anneal_steps: int = 200000, n_epochs: int = 100, weight_decay: float = 0., seed: int = 0,
                 **kwargs):
        super().__init__(hidden, latent, dropout, lr, batch_size, n_epochs, weight_decay, seed, kwargs.get('device'))
        self.anneal_cap, self.total_anneal_steps = float(anneal_cap), int(total_anneal_steps)

    @classmethod
    def shapes(cls, n_items: int, hidden: int, latent: int) -> dict:
        return shapes(n_items, hidden, latent, 2 * latent if cls.VARIATIONAL else latent)

    @property
    def w_enc1(self):
        return None if self.net is None else self.net.w_enc1

    @property
    def code(self) -> int:
        return 2 * self.latent if self.VARIATIONAL else self.latent

    # ---- the network ---------------------------------------------------------------------------------------------------------------
    def encode(self, csr: DeviceCSR, u: torch.Tensor):
        """-> (mu, logvar or None): the encoder over the rows ``u`` of ``csr`` (the normalised rows, or their dropped-out view)"""
        net = self.net
        h = ops.SparseLinearActFn.apply(csr, u, net.w_enc1, net.b_enc1, TANH)
        e = ops.LinearActFn.apply(h, net.w_enc2, net.b_enc2, 0 if self.VARIATIONAL else TANH)
        return (e[:, :self.latent], e[:, self.latent:]) if self.VARIATIONAL else (e, None)

    def decode(self, z: torch.Tensor) -> torch.Tensor:
        net = self.net
        return ops.LinearActFn.apply(ops.LinearActFn.apply(z, net.w_dec1, net.b_dec1, TANH), net.w_dec2, net.b_dec2, 0)

    def _network(self, u: torch.Tensor) -> torch.Tensor:
        return self.decode(self.encode(self._input, u)[0])

    def loss(self, u: torch.Tensor, beta: float = 0., eps: torch.Tensor = None, dropout_seed: int = None, inplace: bool = True):
        """-> (loss, nll, kl, logits) of the batch of users ``u`` (int64 [B] on the device). ``eps`` [B, latent]: Mult-VAE's noise
        (None: ``z = mu``); ``dropout_seed`` None: no input dropout. With ``inplace`` the returned logits are overwritten by their
        gradient when they need one."""
        mu, logvar = self.encode(self._rows_in(dropout_seed), u)
        kl = None
        z = mu
        if self.VARIATIONAL:
            if eps is not None:
                z = mu + eps * torch.exp(0.5 * logvar)
            kl = 0.5 * (-logvar + torch.exp(logvar) + mu * mu - 1).sum(1).mean()
        logits = self.decode(z)
        nll = ops.MultinomialNLLFn.apply(self._matrix, u, logits, inplace, True)
        return (nll + beta * kl if self.VARIATIONAL else nll), nll, kl, logits

    # ---- training ------------------------------------------------------------------------------------------------------------------
    def _batch_loss(self, part: str, u: torch.Tensor, dropout_seed: int) -> torch.Tensor:
        step = self._step
        beta = min(self.anneal_cap, self.anneal_cap * step / self.total_anneal_steps) if self.total_anneal_steps > 0 else self.anneal_cap
        eps = torch.randn(u.numel(), self.latent, generator=self._gen, device=self.device) if self.VARIATIONAL else None
        return self.loss(u, beta, eps, dropout_seed)[0]

    def _epoch(self) -> torch.Tensor:
        """one pass with the one optimizer"""
        return self.train_pass('net')


class MultVAE(MultDAE):
    BINARY_ONLY = 'MultVAE: the multinomial likelihood takes the 0/1 rows as its targets'
    VARIATIONAL = True
