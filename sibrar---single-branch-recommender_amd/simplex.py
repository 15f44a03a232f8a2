"""SimpleX (Mao et al., "SimpleX: A Simple and Strong Baseline for Collaborative Filtering", CIKM 2021; registry name ``simplex``) on the
engine's kernels. The reference has no such model; this one is not a port. The definitions below are the authors' code as remembered, not
a transcription of it.

Two embedding tables ``U`` [n_users, D] and ``V`` [n_items, D] and one D x D map ``W`` without bias. With X the 0/1 users x items
training matrix and ``d_u`` its row degrees, a user is a mix of their own row and the mean of their history:

    p_u = (1 / d_u) sum_{k in X[u]} V[k]          (0 where d_u = 0)
    h_u = gamma * U[u] + (1 - gamma) * (p_u W^T)
    y(u, i) = <h_u, V[i]> / (max(|h_u|, eps) * max(|V[i]|, eps))          eps = ops.COS_EPS

and the cosine contrastive loss of a batch row (u, p, j_1 .. j_N) is

    l = (1 - y(u, p)) + (negative_weight / N) * sum_c max(0, y(u, j_c) - margin),          L = the mean of l over the batch.

The pooling is ``ops.csr_rows_times_dense`` over a resident ``DeviceCSR`` of X whose rows are scaled by ``1 / d_u`` once, the map is
``ops.LinearActFn``, the lookup ``ops.LookupFn``; all stay on the autograd tape, so ``V`` receives the pooling's gradient and the loss's.
The loss is ``ops.CCLLossFn`` on the item table itself (``sbr_ccl_loss_fwd_bwd``: one read of an item row gives the dot product and the
row's norm; ``sbr_scatter_add_cos_rows_sorted`` gathers the table's gradient): no [B, 1 + N, D] copy of item rows or of their gradient,
fixed order, no atomics, valid in deterministic mode (the pooling's gradient takes its fixed-order form when D % 4 == 0).

The model owns its whole objective. In training mode ``forward`` keeps ``{'reg_loss': L, 'pos_loss', 'neg_loss'}`` for
``get_and_reset_other_loss`` and returns the detached cosines [B, 1 + N]; it is configured with ``rec_loss: none``
(``losses.RecNoLoss``), and the loader's ``n_negative_samples`` is N. In evaluation mode the score is the cosine;
``fused_score_transform`` normalises both sides as DeepMF's does, so ``embedding_dim`` 64 / 128 reach the fused scorers. The first two
state_dict keys are ``mf``'s, the third is ``history_linear.weight``: an ``mf`` checkpoint without biases loads with ``strict=False``.

Deliberate differences from the paper: only the mean aggregator is built (the attention aggregators are left out); the history is the
whole training row, not a list truncated to a ``max_len``; there is no embedding dropout; the L2 term is the optimizer's weight decay, as
for every other model here; negatives are the loader's.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import torch
from torch import nn

from . import ops
from .features import DeviceCSR
from .lightgcn import LightGCN

NO_FLOOR = -2.                    # the floor handed to the cosine scorers: below every cosine, so nothing is floored


class SimpleX(LightGCN):
    """``train_matrix``: the users x items training interactions (anything ``scipy.sparse.csr_matrix`` takes), 0/1. ``init_std``: the
    standard deviation of both tables' initial values (None: the base class's initialisation)."""

    def __init__(self, n_users: int, n_items: int, train_matrix, embedding_dim: int = 64, gamma: float = 0.5, margin: float = 0.9,
                 negative_weight: float = 10., init_std=1e-4):
        if not 1 <= embedding_dim <= ops.CCL_MAX_D:
            raise ValueError(f'SimpleX: embedding_dim={embedding_dim} outside [1, {ops.CCL_MAX_D}]')
        if not 0 <= gamma <= 1:
            raise ValueError(f'SimpleX: gamma={gamma} outside [0, 1]')
        if not -1 <= margin <= 1:
            raise ValueError(f'SimpleX: margin={margin} outside [-1, 1], the range of a cosine')
        if not negative_weight >= 0:
            raise ValueError(f'SimpleX: negative_weight={negative_weight} is negative')
        if init_std is not None and not init_std > 0:
            raise ValueError(f'SimpleX: init_std={init_std} is not positive')
        if train_matrix is None:
            raise ValueError('SimpleX: the history pooling needs the training matrix')
        m = sp.csr_matrix(train_matrix)
        if tuple(m.shape) != (n_users, n_items):
            raise ValueError(f'SimpleX: the training matrix is {tuple(m.shape)}, not [{n_users}, {n_items}]')
        m.sum_duplicates()
        if m.nnz and not bool((m.data == 1).all()):
            raise ValueError('SimpleX: the mean of a history is stated for 0/1 interaction data; this matrix has values')
        super().__init__(n_users, n_items, None, embedding_dim=embedding_dim, n_layers=0)      # plain tables: nothing is propagated
        if init_std is not None:
            nn.init.normal_(self.user_embeddings.weight, std=init_std)
            nn.init.normal_(self.item_embeddings.weight, std=init_std)
        self.history_linear = nn.Linear(embedding_dim, embedding_dim, bias=False)
        # X with every row scaled by 1 / d_u, the quotient rounded to float32 once; non-persistent buffers: moves with .to()
        deg = np.diff(m.indptr)
        scale = (1. / np.maximum(deg, 1)).astype(np.float32)
        self._history = DeviceCSR(sp.csr_matrix((np.repeat(scale, deg), m.indices, m.indptr), shape=m.shape))
        self.gamma, self.margin, self.negative_weight = float(gamma), float(margin), float(negative_weight)
        self._kept = None                                         # (L, parts) of the last training forward
        self.name = 'SimpleX'

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        keys = ('embedding_dim', 'gamma', 'margin', 'negative_weight', 'init_std')
        return SimpleX(dataset.n_users, dataset.n_items, dataset.user_sampling_matrix_train, **{k: conf[k] for k in keys if k in conf})

    def _user_rows(self, u_idxs):
        """h [n, D] of the users ``u_idxs`` [n], on the autograd tape"""
        users, items = self._tables()
        if not u_idxs.is_cuda:
            raise RuntimeError('SimpleX (HIP engine) needs CUDA(HIP) index tensors')
        own = ops.LookupFn.apply(users, u_idxs)
        pooled = ops.csr_rows_times_dense(self._history, u_idxs, items)
        mapped = ops.LinearActFn.apply(pooled, self.history_linear.weight, None, 0)
        return self.gamma * own + (1. - self.gamma) * mapped

    def get_user_representations(self, u_idxs):
        return self._user_rows(u_idxs.reshape(-1)).reshape(*u_idxs.shape, self.embedding_dim)

    def combine_user_item_representations(self, u_repr, i_repr):
        if i_repr.ndim == 3 and i_repr.shape[0] == 1:             # [1, I, D]: broadcast over users, as in SGDMatrixFactorization
            i_repr = i_repr[0]
        if i_repr.ndim == 2:
            return ops.score_cos_all(u_repr, i_repr, NO_FLOOR)
        return ops.ScoreCosFn.apply(u_repr, i_repr, NO_FLOOR)

    def fused_score_transform(self):
        """``(items_fn, users_fn, finish_fn)`` for the fused full-catalogue scorers, which compute plain dot products: both sides are
        row-normalised with eps ``ops.COS_EPS`` first, as DeepMF's are, so the dot product IS the cosine; there is no floor to apply."""
        return ops.l2_normalize_rows, ops.l2_normalize_rows, None

    def forward(self, u_idxs, i_idxs):
        if not i_idxs.is_cuda:
            raise RuntimeError('SimpleX (HIP engine) needs CUDA(HIP) index tensors')
        if not self.training:
            return self.combine_user_item_representations(self.get_user_representations(u_idxs), self.get_item_representations(i_idxs))
        if i_idxs.dim() != 2 or u_idxs.dim() != 1 or i_idxs.shape[1] < 2:
            raise ValueError(f'SimpleX: a training batch is u_idxs [B] and i_idxs [B, 1 + N], N >= 1, with the positive in column 0, got '
                             f'{tuple(u_idxs.shape)} and {tuple(i_idxs.shape)}')
        h = self._user_rows(u_idxs)
        loss, parts, scores = ops.CCLLossFn.apply(h, self._tables()[1], i_idxs, self.margin, self.negative_weight)
        self._kept = (loss, parts)
        return scores

    def get_and_reset_other_loss(self):
        kept, self._kept = self._kept, None
        if kept is None:
            zero = torch.zeros((), device=self.device)
            return {'reg_loss': zero, 'pos_loss': zero, 'neg_loss': zero}
        loss, parts = kept
        return {'reg_loss': loss, 'pos_loss': parts[0], 'neg_loss': parts[1]}
