"""DirectAU (Wang et al., "Towards Representation Alignment and Uniformity in Collaborative Filtering", KDD 2022; registry name
``directau``) on the engine's kernels. The reference has no such model; this one is not a port.

An embedding encoder trained without negative samples. With ``u^``, ``i^`` the L2-normalised representations of a batch's users and of
their positive items,

    l_align      = mean_b |u^_b - i^_b|^2
    l_uniform(X) = log( mean_{i<j} exp(-t |x^_i - x^_j|^2) )
    loss         = l_align + gamma * (l_uniform(U^) + l_uniform(I^)) / 2.

The encoder is ``LightGCN``: ``n_layers = 0`` is plain matrix factorisation bit for bit (and then needs no training matrix), the
state_dict keys are ``mf``'s, so ``mf`` checkpoints without biases and ``lightgcn`` checkpoints load, and ``drop_propagated`` and the
eval-mode table cache are inherited. The uniformity term is ``ops.UniformityFn`` (``sbr_uniformity_fwd`` / ``_bwd``: pair weights formed
on chip, nothing of size B x B written, fixed order, valid in deterministic mode), over the B user rows and the B positive-item rows of
the batch, repeated users and items included, as in the authors' code.

In training mode ``forward`` returns the COSINE logits ``u^ . i^`` [B, 1 + N] and keeps ``gamma * (l_uniform(U^) + l_uniform(I^)) / 2``
for ``get_and_reset_other_loss``. With ``rec_loss = align`` (``losses.RecAlignmentLoss``: ``2 - 2 z`` at the positives, the negative
columns ignored) the ``Trainer``'s ``train/rec_loss`` is ``l_align`` and ``train/reg_loss`` the weighted uniformity. In evaluation mode
the representations are the raw encoder rows and the score is their dot product, as in the authors' code: training logits are cosines,
evaluation scores are not. ``embedding_dim`` 64 / 128 therefore reach the fused scorers exactly as ``mf`` and ``lightgcn`` do.

Deliberate differences from the paper: its separate weight decay is the optimizer's; any other ``rec_loss`` on the cosine logits (bpr +
uniformity) works and is not a published model.
"""
from __future__ import annotations

import torch

from . import ops
from .lightgcn import LightGCN

MAX_T = 16.0                      # unit rows: t * max d^2 = 4 t stays inside the uniformity kernel's defined domain (below 80)


class DirectAU(LightGCN):
    """``gamma``: the weight of the uniformity term; ``t``: its temperature, in (0, 16]; ``train_matrix``: the users x items training
    interactions, needed for ``n_layers > 0`` only."""

    def __init__(self, n_users: int, n_items: int, embedding_dim: int = 64, gamma: float = 1.0, t: float = 2.0, n_layers: int = 0,
                 train_matrix=None):
        if not 1 <= embedding_dim <= ops.UNIFORMITY_MAX_D:
            raise ValueError(f'DirectAU: embedding_dim={embedding_dim} outside [1, {ops.UNIFORMITY_MAX_D}]')
        if not gamma >= 0:
            raise ValueError(f'DirectAU: gamma={gamma} is negative')
        if not 0 < t <= MAX_T:
            raise ValueError(f'DirectAU: t={t} outside (0, {MAX_T:g}]')
        if n_layers > 0 and train_matrix is None:
            raise ValueError(f'DirectAU: n_layers={n_layers} needs the training matrix')
        super().__init__(n_users, n_items, train_matrix if n_layers > 0 else None, embedding_dim=embedding_dim, n_layers=n_layers)
        self.gamma, self.t = float(gamma), float(t)
        self._uniform = None                                      # (weighted term, l_uniform(U^), l_uniform(I^)) of the last training forward
        self.name = 'DirectAU'

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        n_layers = conf.get('n_layers', 0)
        return DirectAU(dataset.n_users, dataset.n_items, embedding_dim=conf.get('embedding_dim', 64), gamma=conf.get('gamma', 1.0),
                        t=conf.get('t', 2.0), n_layers=n_layers,
                        train_matrix=dataset.user_sampling_matrix_train if n_layers > 0 else None)

    def forward(self, u_idxs, i_idxs):
        if not self.training:
            return super().forward(u_idxs, i_idxs)
        if not i_idxs.is_cuda:
            raise RuntimeError('DirectAU (HIP engine) needs CUDA(HIP) index tensors')
        if i_idxs.dim() != 2 or u_idxs.dim() != 1:
            raise ValueError(f'DirectAU: a training batch is u_idxs [B] and i_idxs [B, 1 + N] with the positive in column 0, got '
                             f'{tuple(u_idxs.shape)} and {tuple(i_idxs.shape)}')
        users, items = self._tables()                             # one propagation for both sides
        u = ops.L2NormalizeFn.apply(ops.LookupFn.apply(users, u_idxs))
        i_raw = ops.LookupFn.apply(items, i_idxs)
        B, n1, D = i_raw.shape
        i = ops.L2NormalizeFn.apply(i_raw.reshape(B * n1, D)).view(B, n1, D)
        with torch.set_grad_enabled(self.gamma > 0 and torch.is_grad_enabled()):      # gamma = 0: the terms are figures, not objectives
            lu = ops.UniformityFn.apply(u, self.t)
            li = ops.UniformityFn.apply(i[:, 0], self.t)
            self._uniform = (self.gamma * (lu + li) / 2, lu.detach(), li.detach())
        return self.combine_user_item_representations(u, i)

    def get_and_reset_other_loss(self):
        kept, self._uniform = self._uniform, None
        if kept is None:
            zero = torch.zeros((), device=self.device)
            kept = (zero, zero, zero)
        return {'reg_loss': kept[0], 'uniform_u': kept[1], 'uniform_i': kept[2]}
