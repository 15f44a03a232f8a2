"""The simplified ProtoMF models on the engine's kernels — algorithms/sgd_alg.py:643-888, registry names ``uprotomfs``, ``iprotomfs``,
``uiprotomfs`` (algorithms/algorithms_utils.py:30-32), and ``UIProtoMFsCombine``. They are ProtoMF (protomf.py) without regularisers,
with the plain cosine ``clamp(x^ . y^, -1, 1)`` (compute_cosine_sim, sgd_alg.py:62-73) instead of the shifted one, and with a ReLU on the
other entity's weights.

A training forward pass is ONE op per prototype side, ``ops.ProtoScoreFn`` (csrc/proto_cos.hip): embedding lookup, both
normalisations, the cosine, the clamp, the gather of the other entity's weights, their ReLU and the dot over the prototypes; neither the
similarity matrix's inputs nor the ``[B, N + 1, P]`` weight gather is written. ``get_user_representations`` /
``get_item_representations`` / ``combine_user_item_representations`` are the composed route (``ops.ProtoCosFn``, ``ops.LookupFn`` +
ReLU, ``ops.ScoreDotFn`` / ``ops.ScoreAllFn``) that evaluation goes through; both routes are differentiable. state_dict keys, their
order, constructor arguments, configuration keys and initialisation are the reference's.
"""
from __future__ import annotations

from typing import Dict

import torch
from torch import nn

from . import ops
from .protomf import prototype_stats
from .sbnet import SGDBasedRecommenderAlgorithm, general_weight_init


def protomfs_post_val(prototypes: torch.Tensor, entity_embeddings: torch.Tensor, other_weights: torch.Tensor) -> Dict[str, float]:
    """The scalar entries of explanations/utils.py:260-300: ``prototype_stats`` with the plain cosine and ``other_weights``, the relu'd
    weights of the other entity. The images and the t-SNE are left out."""
    return prototype_stats(ops.ProtoCosFn.apply, prototypes, entity_embeddings, other_weights)


class _ProtoSideS(SGDBasedRecommenderAlgorithm):
    """What UProtoMFs and IProtoMFs share: the prototypes and the initialisation of the weight side."""

    def __init__(self, n_users: int, n_items: int, embedding_dim: int, n_prototypes: int):
        super().__init__()
        self.n_users, self.n_items = n_users, n_items
        self.embedding_dim, self.n_prototypes = embedding_dim, n_prototypes

    def _init(self, proto_side: nn.Embedding, weight_side: nn.Embedding):
        self.relu = nn.ReLU()
        self.prototypes = nn.Parameter(torch.randn([self.n_prototypes, self.embedding_dim]) * .1 / self.embedding_dim, requires_grad=True)
        proto_side.apply(general_weight_init)
        torch.nn.init.trunc_normal_(weight_side.weight, mean=0.5, std=.1 / self.embedding_dim, a=0, b=1)

    def combine_user_item_representations(self, u_repr, i_repr):
        return ops.score(u_repr, i_repr)


class UProtoMFs(_ProtoSideS):
    """algorithms/sgd_alg.py:643-702 — user prototypes, relu'd item weights."""

    def __init__(self, n_users: int, n_items: int, embedding_dim: int = 100, n_prototypes: int = 20):
        super().__init__(n_users, n_items, embedding_dim, n_prototypes)
        self.user_embed = nn.Embedding(self.n_users, self.embedding_dim)
        self.item_embed = nn.Embedding(self.n_items, self.n_prototypes)
        self._init(self.user_embed, self.item_embed)
        self.name = 'UProtoMFs'

    def forward(self, u_idxs, i_idxs):
        fan = i_idxs.numel() // max(u_idxs.numel(), 1)
        out = ops.ProtoScoreFn.apply(self.user_embed.weight, u_idxs, self.prototypes, self.item_embed.weight, i_idxs.reshape(-1), fan)
        return out.view(i_idxs.shape)

    def get_user_representations(self, u_idxs):
        return ops.ProtoCosFn.apply(self.user_embed.weight, u_idxs, self.prototypes)     # [batch_size, n_prototypes]

    def get_item_representations(self, i_idxs):
        return self.relu(ops.LookupFn.apply(self.item_embed.weight, i_idxs))              # [batch_size, n_neg + 1, n_prototypes]

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        return UProtoMFs(dataset.n_users, dataset.n_items, conf['embedding_dim'], conf['n_prototypes'])

    def post_val(self, curr_epoch: int):
        return protomfs_post_val(self.prototypes, self.user_embed.weight, self.relu(self.item_embed.weight.detach()))


class IProtoMFs(_ProtoSideS):
    """algorithms/sgd_alg.py:705-765 — item prototypes, relu'd user weights."""

    def __init__(self, n_users: int, n_items: int, embedding_dim: int = 100, n_prototypes: int = 20):
        super().__init__(n_users, n_items, embedding_dim, n_prototypes)
        self.user_embed = nn.Embedding(self.n_users, self.n_prototypes)
        self.item_embed = nn.Embedding(self.n_items, self.embedding_dim)
        self._init(self.item_embed, self.user_embed)
        self.name = 'IProtoMFs'

    def forward(self, u_idxs, i_idxs):
        fan = i_idxs.numel() // max(u_idxs.numel(), 1)
        out = ops.ProtoScoreFn.apply(self.item_embed.weight, i_idxs.reshape(-1), self.prototypes, self.user_embed.weight,
                                     u_idxs.repeat_interleave(fan), 1)
        return out.view(i_idxs.shape)

    def get_user_representations(self, u_idxs):
        return self.relu(ops.LookupFn.apply(self.user_embed.weight, u_idxs))              # [batch_size, n_prototypes]

    def get_item_representations(self, i_idxs):
        return ops.ProtoCosFn.apply(self.item_embed.weight, i_idxs, self.prototypes)     # [*i_idxs.shape, n_prototypes]

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        return IProtoMFs(dataset.n_users, dataset.n_items, conf['embedding_dim'], conf['n_prototypes'])

    def post_val(self, curr_epoch: int):
        return protomfs_post_val(self.prototypes, self.item_embed.weight, self.relu(self.user_embed.weight.detach()))


class UIProtoMFs(SGDBasedRecommenderAlgorithm):
    """algorithms/sgd_alg.py:768-850 — user and item prototypes; each side's weights are the relu'd projection of the other side's
    embedding into its prototype space."""

    def __init__(self, n_users: int, n_items: int, embedding_dim: int = 100, u_n_prototypes: int = 20, i_n_prototypes: int = 20):
        super().__init__()
        self.n_users, self.n_items, self.embedding_dim = n_users, n_items, embedding_dim
        self.uprotomfs = UProtoMFs(n_users, n_items, embedding_dim, u_n_prototypes)
        self.iprotomfs = IProtoMFs(n_users, n_items, embedding_dim, i_n_prototypes)
        self.u_to_i_proj = nn.Linear(self.embedding_dim, i_n_prototypes, bias=False)     # UProtoMFs -> IProtoMFs
        self.i_to_u_proj = nn.Linear(self.embedding_dim, u_n_prototypes, bias=False)     # IProtoMFs -> UProtoMFs
        self.relu = nn.ReLU()
        self.u_to_i_proj.apply(general_weight_init)
        self.i_to_u_proj.apply(general_weight_init)
        # deleting unused parameters
        del self.uprotomfs.item_embed
        del self.iprotomfs.user_embed
        self.name = 'UIProtoMFs'

    def forward(self, u_idxs, i_idxs):
        # u_sim . relu(i_proj) + relu(u_proj) . i_sim (sgd_alg.py:823-825): one fused op per prototype side, the ReLU inside it
        fan = i_idxs.numel() // max(u_idxs.numel(), 1)
        i_flat = i_idxs.reshape(-1)
        u_table, i_table = self.uprotomfs.user_embed.weight, self.iprotomfs.item_embed.weight
        i_proj = ops.GatherLinearFn.apply(i_table, i_flat, self.i_to_u_proj.weight)                            # [B (N + 1), P_u]
        u_proj = ops.GatherLinearFn.apply(u_table, u_idxs.repeat_interleave(fan), self.u_to_i_proj.weight)     # [B (N + 1), P_i]
        u_dots = ops.ProtoScoreFn.apply(u_table, u_idxs, self.uprotomfs.prototypes, i_proj, None, fan)
        i_dots = ops.ProtoScoreFn.apply(i_table, i_flat, self.iprotomfs.prototypes, u_proj, None, 1)
        return u_dots.view(i_idxs.shape) + i_dots.view(i_idxs.shape)

    def get_user_representations(self, u_idxs):
        u_sim_mtx = self.uprotomfs.get_user_representations(u_idxs)
        u_proj = self.relu(ops.GatherLinearFn.apply(self.uprotomfs.user_embed.weight, u_idxs, self.u_to_i_proj.weight))
        return u_sim_mtx, u_proj

    def get_item_representations(self, i_idxs):
        i_sim_mtx = self.iprotomfs.get_item_representations(i_idxs)
        i_proj = self.relu(ops.GatherLinearFn.apply(self.iprotomfs.item_embed.weight, i_idxs, self.i_to_u_proj.weight))
        return i_sim_mtx, i_proj

    def combine_user_item_representations(self, u_repr, i_repr):
        # u_sim . i_proj + u_proj . i_sim (sgd_alg.py:823-825) as ONE product over the concatenated widths
        u_sim_mtx, u_proj = u_repr
        i_sim_mtx, i_proj = i_repr
        return ops.score(torch.cat([u_sim_mtx, u_proj], dim=-1), torch.cat([i_proj, i_sim_mtx], dim=-1))

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        return UIProtoMFs(dataset.n_users, dataset.n_items, conf['embedding_dim'], conf['u_n_prototypes'], conf['i_n_prototypes'])

    def post_val(self, curr_epoch: int):
        u_table, i_table = self.uprotomfs.user_embed.weight, self.iprotomfs.item_embed.weight
        with torch.no_grad():
            i_proj = self.relu(ops.ScoreAllFn.apply(i_table, self.i_to_u_proj.weight))
            u_proj = self.relu(ops.ScoreAllFn.apply(u_table, self.u_to_i_proj.weight))
        u_post_val = protomfs_post_val(self.uprotomfs.prototypes, u_table, i_proj)
        i_post_val = protomfs_post_val(self.iprotomfs.prototypes, i_table, u_proj)
        return {**{'user_' + k: v for k, v in u_post_val.items()}, **{'item_' + k: v for k, v in i_post_val.items()}}


class UIProtoMFsCombine:
    """algorithms/sgd_alg.py:853-888 — encases a trained UProtoMFs and a trained IProtoMFs; its prediction is the sum of theirs. It is
    not optimised, saved, loaded or built from a configuration."""

    def __init__(self, uprotomfs: UProtoMFs, iprotomfs: IProtoMFs):
        self.uprotomfs = uprotomfs
        self.iprotomfs = iprotomfs
        self.name = 'UIProtoMFsCombine'

    def predict(self, u_idxs: torch.Tensor, i_idxs: torch.Tensor) -> torch.Tensor:
        return self.uprotomfs.predict(u_idxs, i_idxs) + self.iprotomfs.predict(u_idxs, i_idxs)

    def save_model_to_path(self, path: str):
        raise ValueError('UIProtoMFsCombine holds two separately trained models and cannot be saved to a path: save its UProtoMFs and its '
                         'IProtoMFs on their own. To optimise one joint model use UIProtoMF / UIProtoMFs.')

    def load_model_from_path(self, path: str):
        raise ValueError('UIProtoMFsCombine holds two separately trained models and cannot be loaded from a path: load its UProtoMFs and '
                         'its IProtoMFs on their own. To optimise one joint model use UIProtoMF / UIProtoMFs.')

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        raise ValueError('UIProtoMFsCombine is made of two trained models and cannot be built from a configuration. To optimise one '
                         'joint model use UIProtoMF / UIProtoMFs.')
