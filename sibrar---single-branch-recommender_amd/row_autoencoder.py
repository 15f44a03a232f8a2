"""What the autoencoders over a user's interaction row share (Mult-VAE, Mult-DAE, RecVAE): the second resident matrix (the
L2-normalised rows) with its value-dropout view, the initialisation of the weights from a shape table, ``fit`` with its passes over a seeded
permutation of the users that have an interaction, and ``model.npz`` (every array of the shape table, every hyper-parameter).

A model writes: the class-level names below, its constructor's own checks and attributes, ``loss``, and
  ``shapes(cls, n_items, hidden, latent)``  name -> shape of every array of the model, in the order they are drawn;
  ``_batch_loss(part, u, dropout_seed)``    the training loss of the users ``u`` in a pass over ``part``, its noise drawn from ``self._gen``;
  ``_epoch()``                              run the epoch's passes -> what the last ``train_pass`` returned;
  ``_network(u)``                           the score rows of the users ``u``: the network without dropout or noise.
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


def init_weights(shapes: dict, generator: torch.Generator, column_major=(), constants=None) -> dict:
    """-> name -> float32 tensor, drawn on the host from ``generator`` in the order of ``shapes``: a matrix [out, in] is Xavier-normal
    (``randn * sqrt(2 / (out + in))``), a vector ``randn * 0.001``; a name of ``constants`` is filled with its value and draws nothing; a
    name of ``column_major`` is laid out column-major (``SparseLinearActFn``'s layout)."""
    out = {}
    for name, shape in shapes.items():
        if constants and name in constants:
            t = torch.full(shape, float(constants[name]))
        elif len(shape) == 2:
            t = torch.randn(*shape, generator=generator) * math.sqrt(2.0 / (shape[0] + shape[1]))
        else:
            t = torch.randn(*shape, generator=generator) * 0.001
        out[name] = t.t().contiguous().t() if name in column_major else t
    return out


class Weights(nn.Module):
    """the tensors of a dict as parameters of their names, each in the layout it comes in"""

    def __init__(self, tensors: dict):
        super().__init__()
        for name, t in tensors.items():
            setattr(self, name, nn.Parameter(t))


class RowAutoencoder(ResidentMatrixAlgorithm):
    """``kwargs`` of every model: ``device``. ``fit(matrix)`` trains; the attributes named by ``PARTS`` hold the weights afterwards
    (None: not fitted)."""
    WHAT = 'weights'
    HYPER = ()              # the constructor's arguments: what build_from_conf takes from a conf and model.npz records
    OPTIONAL = ()           # those of them that may be None, stored in model.npz as NaN
    PARTS = {}              # attribute -> the names of the shape table that module holds; one FusedOptimizer('adam') each
    INPUT = None            # the first layer's weight [hidden, n_items]: stored column-major, and where model.npz's n_items is read
    CONSTANTS = {}          # name -> the value it is filled with

    def __init__(self, hidden, latent, dropout, lr, batch_size, n_epochs, weight_decay, seed, device=None):
        super().__init__(device)
        if hidden < 1 or latent < 1 or batch_size < 1 or n_epochs < 0:
            raise ValueError(f'hidden={hidden}, latent={latent}, batch_size={batch_size} must be positive and n_epochs={n_epochs} not negative')
        if not 0 <= dropout < 1:
            raise ValueError(f'dropout={dropout!r} outside [0, 1)')
        self.hidden, self.latent, self.dropout, self.lr, self.batch_size = int(hidden), int(latent), float(dropout), float(lr), int(batch_size)
        self.n_epochs, self.weight_decay, self.seed = int(n_epochs), float(weight_decay), int(seed)
        for part in self.PARTS:
            setattr(self, part, None)
        self._input = None                     # the L2-normalised rows
        self._forget_views()
        self.epoch_losses = []
        self.name = type(self).__name__
        logging.info(f'Built {self.name} module \n- hidden: {self.hidden} \n- latent: {self.latent} \n- dropout: {self.dropout} ')

    @classmethod
    def build_from_conf(cls, conf: dict, dataset=None):
        return cls(**{k: conf[k] for k in cls.HYPER if k in conf})

    # ---- residency ---------------------------------------------------------------------------------------------------------------
    def _forget_views(self):
        """drop what was derived from the resident matrices"""
        self._dropped = self._kept_values = None            # the value view for the input dropout, and the values it started with

    def _resident(self, m: sp.csr_matrix) -> DeviceCSR:
        self._input = DeviceCSR(m, l2_normalize_rows=True).to(self.device)
        self._forget_views()
        return DeviceCSR(m)

    def to(self, device):
        super().to(device)
        if self._input is not None:
            self._input = self._input.to(self.device)
        self._forget_views()
        for part in self.PARTS:
            if getattr(self, part) is not None:
                setattr(self, part, getattr(self, part).to(self.device))
        return self

    def dropped_input(self, seed: int) -> DeviceCSR:
        """the normalised rows with ``sbr_dropout(p = dropout, seed)`` applied to their stored values"""
        if self._dropped is None:
            self._dropped = self._input.value_view()
            self._kept_values = self._dropped.data
        return self._dropped.replace_values(ops.DropoutFn.apply(self._kept_values, self.dropout, int(seed)))

    def _rows_in(self, dropout_seed) -> DeviceCSR:
        """the input of a forward pass; ``dropout_seed`` None: no input dropout"""
        return self.dropped_input(dropout_seed) if dropout_seed is not None and self.dropout > 0 else self._input

    def _set_weights(self, tensors: dict):
        """take the arrays of the shape table as the model's, on its device"""
        for part, names in self.PARTS.items():
            setattr(self, part, Weights({k: tensors[k] for k in names}).to(self.device))

    # ---- training ------------------------------------------------------------------------------------------------------------------
    def fit(self, matrix: sp.spmatrix, **kwargs):
        """:param matrix: user x item sparse matrix, 0/1"""
        self.attach(matrix)
        for part in self.PARTS:
            setattr(self, part, None)
        self._set_weights(init_weights(self.shapes(self.n_items, self.hidden, self.latent), torch.Generator().manual_seed(self.seed),
                                       (self.INPUT,), self.CONSTANTS))
        self._opts = {part: FusedOptimizer(getattr(self, part), 'adam', self.lr, self.weight_decay) for part in self.PARTS}
        self._gen = torch.Generator(device=self.device).manual_seed(self.seed)
        counts = self._matrix.indptr[1:] - self._matrix.indptr[:-1]
        self._active = torch.nonzero(counts > 0).reshape(-1)
        self._step, self.epoch_losses = 0, []
        for epoch in range(self.n_epochs):
            self.train_epoch()
            logging.info(f'{self.name}: epoch {epoch} loss {self.epoch_losses[-1]:.6f}')
        return self

    def train_pass(self, part: str) -> torch.Tensor:
        """One pass over a fresh permutation of the users that have an interaction, updating ``part`` -> the sum of the batch losses
        times the batch sizes, on the device (no synchronisation)."""
        opt = self._opts[part]
        order = self._active[torch.randperm(self._active.numel(), generator=self._gen, device=self.device)]
        total = torch.zeros((), device=self.device)
        for lo in range(0, order.numel(), self.batch_size):
            u = order[lo:lo + self.batch_size].contiguous()
            loss = self._batch_loss(part, u, (self.seed << 32) + self._step)          # a fresh dropout seed per optimizer step
            loss.backward()
            opt.step()
            opt.zero_grad()
            total += loss.detach() * u.numel()
            self._step += 1
        return total

    def train_epoch(self) -> float:
        """One epoch (after ``fit`` has set the training state up, also with ``n_epochs=0``) -> the mean loss of its last pass, which is
        also appended to ``epoch_losses``: the epoch's one synchronisation."""
        self.epoch_losses.append(float(self._epoch()) / max(self._active.numel(), 1))
        return self.epoch_losses[-1]

    # ---- scoring -------------------------------------------------------------------------------------------------------------------
    def _arrays(self) -> dict:
        return {k: getattr(getattr(self, part), k) for part, names in self.PARTS.items() for k in names}

    @torch.no_grad()
    def _score_rows(self, u: torch.Tensor) -> torch.Tensor:
        n_items = self._arrays()[self.INPUT].shape[1]
        if n_items != self.n_items:
            raise ValueError(f'{self.name}: weights for {n_items} items do not fit the {self.n_items} items of the matrix')
        return self._network(u.long().contiguous())

    # ---- persistence ---------------------------------------------------------------------------------------------------------------
    def _npz_fields(self) -> dict:
        hyper = {h: np.array(np.nan if getattr(self, h) is None else getattr(self, h)) for h in self.HYPER}      # None (OPTIONAL) is stored as NaN
        return {**{k: v.detach().cpu().numpy() for k, v in self._arrays().items()}, **hyper}

    def _read_npz(self, f):
        params = tuple(k for names in self.PARTS.values() for k in names)
        missing = [k for k in params + tuple(self.HYPER) if k not in f.files]
        if missing:
            raise ValueError(f'model.npz: no {missing}')
        hyper = {h: f[h].item() for h in self.HYPER}
        w = {k: f[k] for k in params}
        hidden, latent = int(hyper['hidden']), int(hyper['latent'])
        want = self.shapes(w[self.INPUT].shape[1] if w[self.INPUT].ndim == 2 else -1, hidden, latent)
        bad = {k: w[k].shape for k in params if tuple(w[k].shape) != want[k]}
        if bad:
            raise ValueError(f'model.npz: arrays of shapes {bad} do not belong to a {self.name} with hidden={hidden}, latent={latent}')
        tensors = {k: torch.from_numpy(np.ascontiguousarray(w[k], dtype=np.float32)) for k in params}
        tensors[self.INPUT] = tensors[self.INPUT].t().contiguous().t()
        for h in self.HYPER:
            if h in self.OPTIONAL:
                setattr(self, h, None if math.isnan(hyper[h]) else float(hyper[h]))
            else:
                setattr(self, h, type(getattr(self, h))(hyper[h]))
        self._set_weights(tensors)
