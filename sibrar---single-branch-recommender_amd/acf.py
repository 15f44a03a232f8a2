"""ACF — Anchor-based Collaborative Filtering (Barkan et al., CIKM 2021) on the engine's kernels — algorithms/sgd_alg.py:203-329, registry
name ``acf``; the baseline ProtoMF is compared with, behind the same plugin surface (PrototypeWrapper). A user and an item are both
represented by a softmax mixture of a small set of learned anchors shared by the two sides.

Each side of a forward pass is ONE op, ``ops.AnchorMixFn`` (csrc/anchor_mix.hip): embedding lookup, the logits against the anchors, the
softmax, the mixture and — on the item side — the exclusiveness and inclusiveness entropies of ACF.forward; the score is the per-slot dot
``ops.ScoreDotFn`` in training and the all-pairs ``ops.ScoreAllFn`` in evaluation. state_dict keys, their order, constructor arguments,
configuration keys and loss-dictionary keys are the reference's. The regulariser values stay on the device: ``get_and_reset_other_loss``
never synchronises.

One deviation: the logits are never materialised, so the third entry of the item representation (``c_i_unnorm`` in the reference) is
``None`` here; nothing in the reference reads it outside ACF.forward, whose entropy the kernel computes itself.
"""
from __future__ import annotations

from typing import Dict

import torch
from torch import nn

from . import ops
from .protomf import PrototypeWrapper, prototype_stats


def acf_post_val_light(anchors: torch.Tensor, entity_embeddings: torch.Tensor) -> Dict[str, float]:
    """``prototype_stats`` with sim_func = compute_cosine_sim (sgd_alg.py:62-73, 322-329) on the anchors: the plain cosine clamped to
    [-1, 1], the un-clamped one ``sbr_proto_sim_fwd`` writes next to ProtoMF's shifted similarity."""
    return prototype_stats(ops.cosine_sim, anchors, entity_embeddings)


class ACF(PrototypeWrapper):
    """algorithms/sgd_alg.py:203-329."""

    def __init__(self, n_users: int, n_items: int, embedding_dim: int = 100, n_anchors: int = 20, delta_exc: float = 1e-1,
                 delta_inc: float = 1e-2):
        super().__init__()
        self.n_users, self.n_items = n_users, n_items
        self.embedding_dim, self.n_anchors = embedding_dim, n_anchors
        self.delta_exc, self.delta_inc = delta_exc, delta_inc
        # NB (the reference's): for stability ACF's weights must NOT be initialised with small values — nn.Embedding's own N(0, 1)
        # stays, general_weight_init is deliberately not applied
        self.anchors = nn.Parameter(torch.randn([self.n_anchors, self.embedding_dim]), requires_grad=True)
        self.user_embed = nn.Embedding(self.n_users, self.embedding_dim)
        self.item_embed = nn.Embedding(self.n_items, self.embedding_dim)
        self._acc_exc = 0
        self._acc_inc = 0
        self.name = 'ACF'

    def _mix(self, table: torch.Tensor, idxs: torch.Tensor, with_losses: bool):
        if not idxs.is_cuda:
            raise RuntimeError(f'{self.name} (HIP engine) needs CUDA(HIP) index tensors')
        return ops.AnchorMixFn.apply(table, idxs, self.anchors, with_losses)

    def forward(self, u_idxs, i_idxs):
        u_anc, _, _, _ = self._mix(self.user_embed.weight, u_idxs, False)
        i_anc, c_i, exc_loss, inc_loss = self._mix(self.item_embed.weight, i_idxs, True)
        dots = self.combine_user_item_representations(u_anc, (i_anc, c_i, None))
        self._acc_exc += exc_loss
        self._acc_inc += inc_loss
        return dots

    def get_user_representations(self, u_idxs):
        return self._mix(self.user_embed.weight, u_idxs, False)[0]                      # [batch_size, embedding_dim]

    def get_item_representations(self, i_idxs):
        """-> (i_anc, c_i, None): the reference's third entry, the logits ``c_i_unnorm``, is never materialised."""
        i_anc, c_i, _, _ = self._mix(self.item_embed.weight, i_idxs, False)
        return i_anc, c_i, None

    def combine_user_item_representations(self, u_repr, i_repr):
        # i_anc [B, N, D] in training, [I, D] in evaluation (eval/eval.py:209-217)
        return ops.score(u_repr, i_repr[0])

    def fused_score_transform(self):
        """The score is the plain dot product of ``u_anc`` and ``i_anc``: the fused scorers take the first entry of the item tuple."""
        return (lambda i_repr: i_repr[0]), None, None

    def _coefficients(self, table, idxs):
        if not idxs.is_cuda:
            raise RuntimeError(f'{self.name} (HIP engine) needs CUDA(HIP) index tensors')
        return ops.anchor_mix(table, idxs, self.anchors, want='c')

    def _mixture(self, c):
        # c @ anchors on stored coefficients (sgd_alg.py:291-303): a plain GEMM, no autograd
        if not c.is_cuda:
            raise RuntimeError(f'{self.name} (HIP engine) needs CUDA(HIP) tensors')
        flat = c.detach().reshape(-1, self.n_anchors).float().contiguous()
        return ops.matmul_nn(flat, self.anchors.detach()).view(*c.shape[:-1], self.embedding_dim)

    def get_item_representations_pre_tune(self, i_idxs):
        return self._coefficients(self.item_embed.weight, i_idxs)

    def get_item_representations_post_tune(self, c_i):
        return self._mixture(c_i), c_i, None

    def get_user_representations_pre_tune(self, u_idxs):
        return self._coefficients(self.user_embed.weight, u_idxs)

    def get_user_representations_post_tune(self, c_u):
        return self._mixture(c_u)

    def get_and_reset_other_loss(self) -> Dict:
        acc_exc, acc_inc = self._acc_exc, self._acc_inc
        self._acc_exc = self._acc_inc = 0
        exc_loss = self.delta_exc * acc_exc
        inc_loss = self.delta_inc * acc_inc
        return {'reg_loss': exc_loss + inc_loss, 'exc_loss': exc_loss, 'inc_loss': inc_loss}

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        return ACF(dataset.n_users, dataset.n_items, conf['embedding_dim'], conf['n_anchors'], conf['delta_exc'], conf['delta_inc'])

    def post_val(self, curr_epoch: int):
        return acf_post_val_light(self.anchors, self.item_embed.weight)
