"""UltraGCN (Mao et al., "UltraGCN: Ultra Simplification of Graph Convolutional Networks for Recommendation", CIKM 2021; registry name
``ultragcn``) on the engine's kernels. The reference has no such model; this one is not a port. The definitions below are the authors'
code as remembered, not a transcription of it.

No message passing at all: two plain embedding tables, trained on a degree-weighted pointwise loss over a positive and N sampled
negatives per batch row, plus a term that pulls the user towards the K items that co-occur most with the positive. With X the 0/1
users x items training matrix, ``d_u`` / ``d_i`` its degrees, ``G = X^T X`` (diagonal included) and ``g_i = sum_j G_ij``:

    beta_u = sqrt(d_u + 1) / d_u  (0 where d_u = 0)            beta_i = 1 / sqrt(d_i + 1)
    omega_ij = G_ij * (sqrt(g_i + 1) / g_i) * (1 / sqrt(g_j + 1))
    nbr[i] = the K largest omega_ij with G_ij > 0 by (value descending, index ascending), item i itself included

and for a batch row (u, p, j_1 .. j_N), with ``s(i) = <U[u], V[i]>`` and ``sp`` the overflow-safe softplus,

    L_pos = (w1 + w2 beta_u beta_p) sp(-s(p))          L_neg = (1 / N) sum_c (w3 + w4 beta_u beta_jc) sp(s(j_c))
    L_nbr = sum_{k < len[p]} omega[p, k] sp(-s(nbr[p, k]))
    L = sum over the batch of (L_pos + negative_weight * L_neg + lam * L_nbr)                 (a sum, not a mean)

The lists come from ``ops.cooc_weight_topk`` (``sbr_cooc_weight_topk``: counting, value and selection of one item's row inside one
workgroup, nothing of size items x items), the scale vectors from ``ops.ultragcn_scales``; both are built once, the first time the model
needs them on its device (a model is constructed on the host, and the package has no host path), and then move with the model. A training
step is ``ops.LookupFn`` on the user table and ``ops.UltraGCNLossFn`` on the item table itself: no [B, 1 + N + K, D] copy of item rows
or of their gradient, fixed order, no atomics, valid in deterministic mode.

The model owns its whole objective. In training mode ``forward`` keeps ``{'reg_loss': L, 'pos_loss', 'neg_loss', 'nbr_loss'}`` for
``get_and_reset_other_loss`` and returns the detached scores [B, 1 + N]; it is configured with ``rec_loss: none``
(``losses.RecNoLoss``, a zero), and the loader's ``n_negative_samples`` is N. In evaluation mode everything is ``mf``'s: the score is the
dot product, so ``embedding_dim`` 64 / 128 reach the fused scorers. The state_dict keys are ``mf``'s; ``mf`` checkpoints without biases
load.

Deliberate differences from the paper: its L2 term over all parameters is the optimizer's weight decay, as for every other model here;
negatives are the loader's (which avoids the user's positives), not the authors' sampler.
"""
from __future__ import annotations

import torch
from torch import nn

from . import ops
from .features import DeviceCSR
from .lightgcn import LightGCN


class UltraGCN(LightGCN):
    """``train_matrix``: the users x items training interactions (anything ``scipy.sparse.csr_matrix`` takes), 0/1."""

    def __init__(self, n_users: int, n_items: int, train_matrix, embedding_dim: int = 64, n_neighbors: int = 10, w1: float = 1e-6,
                 w2: float = 1., w3: float = 1e-6, w4: float = 1., negative_weight: float = 300., lam: float = 5e-4, init_std: float = 1e-4):
        if not 1 <= embedding_dim <= ops.ULTRAGCN_MAX_D:
            raise ValueError(f'UltraGCN: embedding_dim={embedding_dim} outside [1, {ops.ULTRAGCN_MAX_D}]')
        if not 1 <= n_neighbors <= ops.COOC_MAX_K:
            raise ValueError(f'UltraGCN: n_neighbors={n_neighbors} outside [1, {ops.COOC_MAX_K}]')
        for name, v in (('w1', w1), ('w2', w2), ('w3', w3), ('w4', w4), ('negative_weight', negative_weight), ('lam', lam)):
            if not v >= 0:
                raise ValueError(f'UltraGCN: {name}={v} is negative')
        if not init_std > 0:
            raise ValueError(f'UltraGCN: init_std={init_std} is not positive')
        if train_matrix is None:
            raise ValueError('UltraGCN: the degree weights and the neighbour lists need the training matrix')
        super().__init__(n_users, n_items, None, embedding_dim=embedding_dim, n_layers=0)      # plain tables: nothing is propagated
        nn.init.normal_(self.user_embeddings.weight, std=init_std)
        nn.init.normal_(self.item_embeddings.weight, std=init_std)
        self._matrix = DeviceCSR(train_matrix)                   # needed until the lists are built; moves with .to()
        if tuple(self._matrix.shape) != (n_users, n_items):
            raise ValueError(f'UltraGCN: the training matrix is {tuple(self._matrix.shape)}, not [{n_users}, {n_items}]')
        if self._matrix.data is not None:
            raise ValueError('UltraGCN: degrees and co-occurrence counts are stated for 0/1 interaction data; this matrix has values')
        self.n_neighbors = int(n_neighbors)
        self.w1, self.w2, self.w3, self.w4 = float(w1), float(w2), float(w3), float(w4)
        self.negative_weight, self.lam = float(negative_weight), float(lam)
        for name in ('beta_u', 'beta_i', 'nbr_idx', 'nbr_val', 'nbr_len'):                      # non-persistent: rebuilt from the matrix
            self.register_buffer(name, None, persistent=False)
        self._kept = None                                         # (L, parts) of the last training forward
        self.name = 'UltraGCN'

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        keys = ('embedding_dim', 'n_neighbors', 'w1', 'w2', 'w3', 'w4', 'negative_weight', 'lam', 'init_std')
        return UltraGCN(dataset.n_users, dataset.n_items, dataset.user_sampling_matrix_train, **{k: conf[k] for k in keys if k in conf})

    def constraints(self):
        """-> (beta_u, beta_i, nbr_idx, nbr_val, nbr_len) on the model's device; built on first use, once"""
        if self.nbr_idx is None:
            if not self.item_embeddings.weight.is_cuda:
                raise RuntimeError('UltraGCN (HIP engine) needs its parameters on a CUDA(HIP) device')
            csr = self._matrix.to(self.item_embeddings.weight.device)
            self.beta_u, self.beta_i, row_scale, col_scale = ops.ultragcn_scales(csr)
            self.nbr_idx, self.nbr_val, self.nbr_len = ops.cooc_weight_topk(csr, row_scale, col_scale, self.n_neighbors, include_self=True)
            self._matrix = None
        return self.beta_u, self.beta_i, self.nbr_idx, self.nbr_val, self.nbr_len

    def forward(self, u_idxs, i_idxs):
        if not self.training:
            return super().forward(u_idxs, i_idxs)
        if not i_idxs.is_cuda:
            raise RuntimeError('UltraGCN (HIP engine) needs CUDA(HIP) index tensors')
        if i_idxs.dim() != 2 or u_idxs.dim() != 1 or i_idxs.shape[1] < 2:
            raise ValueError(f'UltraGCN: a training batch is u_idxs [B] and i_idxs [B, 1 + N], N >= 1, with the positive in column 0, got '
                             f'{tuple(u_idxs.shape)} and {tuple(i_idxs.shape)}')
        users, items = self._tables()
        ub = ops.LookupFn.apply(users, u_idxs)
        loss, parts, scores = ops.UltraGCNLossFn.apply(ub, items, u_idxs, i_idxs, *self.constraints(), self.w1, self.w2, self.w3, self.w4,
                                                       self.negative_weight, self.lam)
        self._kept = (loss, parts)
        return scores

    def get_and_reset_other_loss(self):
        kept, self._kept = self._kept, None
        if kept is None:
            zero = torch.zeros((), device=self.device)
            return {'reg_loss': zero, 'pos_loss': zero, 'neg_loss': zero, 'nbr_loss': zero}
        loss, parts = kept
        return {'reg_loss': loss, 'pos_loss': parts[0], 'neg_loss': parts[1], 'nbr_loss': parts[2]}
