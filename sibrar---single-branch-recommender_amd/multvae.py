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

import logging
import math

import numpy as np
import scipy.sparse as sp
import torch
from torch import nn

from . import ops
from .features import DeviceCSR
from .matrix_models import ResidentMatrixAlgorithm
from .optim import FusedOptimizer

TANH = ops.ACT_CODES['tanh']
PARAMS = ('w_enc1', 'b_enc1', 'w_enc2', 'b_enc2', 'w_dec1', 'b_dec1', 'w_dec2', 'b_dec2')
HYPER = ('hidden', 'latent', 'dropout', 'lr', 'batch_size', 'anneal_cap', 'total_anneal_steps', 'n_epochs', 'weight_decay', 'seed')


class AutoencoderWeights(nn.Module):
    """The eight parameters: ``w_enc1`` [hidden, I] stored column-major (``SparseLinearActFn``'s layout), ``w_enc2`` [code, hidden] with
    code = 2 * latent (Mult-VAE) or latent (Mult-DAE), ``w_dec1`` [hidden, latent], ``w_dec2`` [I, hidden], and their biases. Weights
    are Xavier-normal, biases normal with std 0.001, drawn on the host from ``seed``."""

    def __init__(self, n_items: int, hidden: int, latent: int, code: int, seed: int = 0):
        super().__init__()
        g = torch.Generator().manual_seed(int(seed))
        for name, (out, inp) in zip(('enc1', 'enc2', 'dec1', 'dec2'), ((hidden, n_items), (code, hidden), (hidden, latent), (n_items, hidden))):
            w = torch.randn(out, inp, generator=g) * math.sqrt(2.0 / (out + inp))
            if name == 'enc1':
                w = w.t().contiguous().t()
            setattr(self, 'w_' + name, nn.Parameter(w))
            setattr(self, 'b_' + name, nn.Parameter(torch.randn(out, generator=g) * 0.001))


class MultDAE(ResidentMatrixAlgorithm):
    """``kwargs``: ``device``. ``fit(matrix)`` trains; ``net`` holds the weights afterwards (None: not fitted)."""
    KEY, WHAT = 'w_enc1', 'weights'
    STORES = 'the autoencoder\'s eight weight arrays'
    BINARY_ONLY = 'MultDAE: the multinomial likelihood takes the 0/1 rows as its targets'
    VARIATIONAL = False

    def __init__(self, hidden: int = 600, latent: int = 200, dropout: float = 0.5, lr: float = 1e-3, batch_size: int = 500,
                 anneal_cap: float = 0.2, total_anneal_steps: int = 200000, n_epochs: int = 100, weight_decay: float = 0., seed: int = 0,
                 **kwargs):
        super().__init__(kwargs.get('device'))
        if hidden < 1 or latent < 1 or batch_size < 1 or n_epochs < 0:
            raise ValueError(f'hidden={hidden}, latent={latent}, batch_size={batch_size} must be positive and n_epochs={n_epochs} not negative')
        if not 0 <= dropout < 1:
            raise ValueError(f'dropout={dropout!r} outside [0, 1)')
        self.hidden, self.latent, self.dropout, self.lr, self.batch_size = int(hidden), int(latent), float(dropout), float(lr), int(batch_size)
        self.anneal_cap, self.total_anneal_steps = float(anneal_cap), int(total_anneal_steps)
        self.n_epochs, self.weight_decay, self.seed = int(n_epochs), float(weight_decay), int(seed)
        self.net = None
        self._input = self._dropped = None     # the L2-normalised rows, and their value view for the input dropout
        self.epoch_losses = []
        self.name = 'MultVAE' if self.VARIATIONAL else 'MultDAE'
        logging.info(f'Built {self.name} module \n- hidden: {self.hidden} \n- latent: {self.latent} \n- dropout: {self.dropout} ')

    @classmethod
    def build_from_conf(cls, conf: dict, dataset=None):
        return cls(**{k: conf[k] for k in HYPER if k in conf})

    @property
    def w_enc1(self):
        return None if self.net is None else self.net.w_enc1

    @property
    def code(self) -> int:
        return 2 * self.latent if self.VARIATIONAL else self.latent

    # ---- residency ---------------------------------------------------------------------------------------------------------------
    def _resident(self, m: sp.csr_matrix) -> DeviceCSR:
        self._input = DeviceCSR(m, l2_normalize_rows=True).to(self.device)
        self._dropped = None
        return DeviceCSR(m)

    def to(self, device):
        super().to(device)
        if self._input is not None:
            self._input, self._dropped = self._input.to(self.device), None
        if self.net is not None:
            self.net = self.net.to(self.device)
        return self

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

    def dropped_input(self, seed: int) -> DeviceCSR:
        """the normalised rows with ``sbr_dropout(p = dropout, seed)`` applied to their stored values"""
        if self._dropped is None:
            self._dropped = self._input.value_view()
            self._kept_values = self._dropped.data
        return self._dropped.replace_values(ops.DropoutFn.apply(self._kept_values, self.dropout, int(seed)))

    def loss(self, u: torch.Tensor, beta: float = 0., eps: torch.Tensor = None, dropout_seed: int = None, inplace: bool = True):
        """-> (loss, nll, kl, logits) of the batch of users ``u`` (int64 [B] on the device). ``eps`` [B, latent]: Mult-VAE's noise
        (None: ``z = mu``); ``dropout_seed`` None: no input dropout. With ``inplace`` the returned logits are overwritten by their
        gradient when they need one."""
        csr = self.dropped_input(dropout_seed) if dropout_seed is not None and self.dropout > 0 else self._input
        mu, logvar = self.encode(csr, u)
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
    def fit(self, matrix: sp.spmatrix, **kwargs):
        """:param matrix: user x item sparse matrix, 0/1"""
        self.attach(matrix)
        self.net = None
        net = AutoencoderWeights(self.n_items, self.hidden, self.latent, self.code, self.seed).to(self.device)
        self.net = net
        self._opt = FusedOptimizer(net, 'adam', self.lr, self.weight_decay)
        self._gen = torch.Generator(device=self.device).manual_seed(self.seed)
        counts = self._matrix.indptr[1:] - self._matrix.indptr[:-1]
        self._active = torch.nonzero(counts > 0).reshape(-1)
        self._step, self.epoch_losses = 0, []
        for epoch in range(self.n_epochs):
            self.train_epoch()
            logging.info(f'{self.name}: epoch {epoch} loss {self.epoch_losses[-1]:.6f}')
        return self

    def train_epoch(self) -> float:
        """One pass over a fresh permutation of the users that have an interaction (after ``fit`` has set the training state up, also
        with ``n_epochs=0``) -> the epoch's mean loss, which is also appended to ``epoch_losses``: the epoch's one synchronisation."""
        opt, gen = self._opt, self._gen
        order = self._active[torch.randperm(self._active.numel(), generator=gen, device=self.device)]
        total = torch.zeros((), device=self.device)
        for lo in range(0, order.numel(), self.batch_size):
            u = order[lo:lo + self.batch_size].contiguous()
            step = self._step
            beta = min(self.anneal_cap, self.anneal_cap * step / self.total_anneal_steps) if self.total_anneal_steps > 0 else self.anneal_cap
            eps = torch.randn(u.numel(), self.latent, generator=gen, device=self.device) if self.VARIATIONAL else None
            loss = self.loss(u, beta, eps, dropout_seed=(self.seed << 32) + step)[0]
            loss.backward()
            opt.step()
            opt.zero_grad()
            total += loss.detach() * u.numel()
            self._step += 1
        self.epoch_losses.append(float(total) / max(order.numel(), 1))
        return self.epoch_losses[-1]

    # ---- scoring -------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _score_rows(self, u: torch.Tensor) -> torch.Tensor:
        if self.net.w_enc1.shape[1] != self.n_items:
            raise ValueError(f'{self.name}: weights for {self.net.w_enc1.shape[1]} items do not fit the {self.n_items} items of the matrix')
        return self.decode(self.encode(self._input, u.long().contiguous())[0])

    # ---- persistence ---------------------------------------------------------------------------------------------------------------
    def _npz_fields(self) -> dict:
        return {**{k: getattr(self.net, k).detach().cpu().numpy() for k in PARAMS}, **{h: np.array(getattr(self, h)) for h in HYPER}}

    def _read_npz(self, f):
        missing = [k for k in PARAMS + HYPER if k not in f.files]
        if missing:
            raise ValueError(f'model.npz: no {missing}')
        hyper = {h: f[h].item() for h in HYPER}
        w = {k: f[k] for k in PARAMS}
        hidden, latent = int(hyper['hidden']), int(hyper['latent'])
        code = 2 * latent if self.VARIATIONAL else latent
        n_items = w['w_enc1'].shape[1] if w['w_enc1'].ndim == 2 else -1
        want = {'w_enc1': (hidden, n_items), 'b_enc1': (hidden,), 'w_enc2': (code, hidden), 'b_enc2': (code,), 'w_dec1': (hidden, latent),
                'b_dec1': (hidden,), 'w_dec2': (n_items, hidden), 'b_dec2': (n_items,)}
        bad = {k: w[k].shape for k in PARAMS if tuple(w[k].shape) != want[k]}
        if bad:
            raise ValueError(f'model.npz: arrays of shapes {bad} do not belong to a {self.name} with hidden={hidden}, latent={latent}')
        net = AutoencoderWeights(n_items, hidden, latent, code)
        with torch.no_grad():
            for k in PARAMS:
                getattr(net, k).copy_(torch.from_numpy(w[k].astype(np.float32)))
        for h in HYPER:
            setattr(self, h, type(getattr(self, h))(hyper[h]))
        self.net = net.to(self.device)


class MultVAE(MultDAE):
    BINARY_ONLY = 'MultVAE: the multinomial likelihood takes the 0/1 rows as its targets'
    VARIATIONAL = True
