"""ProtoMF (Melchiorre et al., RecSys 2022) on the engine's kernels — algorithms/sgd_alg.py:332-640, registry names ``uprotomf``,
``iprotomf``, ``uiprotomf``; sibling models of SingleBranchNet behind the same plugin surface (algorithms/base_classes.py:173-188:
PrototypeWrapper). An entity is represented by its shifted cosine similarities to a small set of learned prototypes.

The prototype side of a forward pass is ONE op, ``ops.ProtoSimFn`` (csrc/proto_cos.hip): embedding lookup, both normalisations, the
similarity matrix, the clamp and the two arg-min regularisers of ``compute_reg_losses``; the other side is a plain ``ops.LookupFn``, the
per-slot dot ``ops.ScoreDotFn`` and the all-pairs evaluation form ``ops.ScoreAllFn``. UIProtoMF's projections are GEMMs on gathered rows
(``ops.GatherLinearFn``). state_dict keys, their order, constructor arguments, configuration keys and loss-dictionary keys are the
reference's. The regulariser values stay on the device: ``get_and_reset_other_loss`` never synchronises.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import nn

from . import ops
from .sbnet import SGDBasedRecommenderAlgorithm, general_weight_init

MAX_ENTITIES = 10000              # explanations/utils.py:16


class PrototypeWrapper(SGDBasedRecommenderAlgorithm):
    """algorithms/base_classes.py:173-188."""

    def get_item_representations_pre_tune(self, i_idxs):
        raise NotImplementedError('This method has not been implemented for this class!')

    def get_item_representations_post_tune(self, i_repr):
        raise NotImplementedError('This method has not been implemented for this class!')

    def get_user_representations_pre_tune(self, u_idxs):
        raise NotImplementedError('This method has not been implemented for this class!')

    def get_user_representations_post_tune(self, u_repr):
        raise NotImplementedError('This method has not been implemented for this class!')


def prototype_stats(sim, prototypes: torch.Tensor, entity_embeddings: torch.Tensor,
                    other_weights: Optional[torch.Tensor] = None) -> Dict[str, float]:
    """explanations/utils.py:223-257 (and the scalar entries of 260-300) for the similarity ``sim(table, idx, prototypes)``
    (``ops.proto_sim``, ``ops.cosine_sim``, ``ops.ProtoCosFn.apply``), from the two blocks of the similarity matrix they read — prototypes
    x prototypes and entities x prototypes; the (P + n)^2 matrix of the reference is never built. ``other_weights`` (ProtoMFs: the relu'd
    weights of the other entity) adds the means of the non-zero count and of the sum of its rows. From MAX_ENTITIES entities upward a
    random subset is used, as in the reference."""
    n_prototypes = len(prototypes)
    names = ['avg_pairwise_proto_sim', 'entity_to_proto_mean', 'entity_to_proto_max', 'entity_to_proto_min']
    with torch.no_grad():
        idx = None
        if len(entity_embeddings) >= MAX_ENTITIES:
            idx = torch.randperm(len(entity_embeddings))[:MAX_ENTITIES].to(entity_embeddings.device)
        sim_mtx_proto = sim(prototypes, None, prototypes)
        entity_to_proto = sim(entity_embeddings, idx, prototypes)
        sim_mtx_proto_tril = torch.tril(sim_mtx_proto, diagonal=-1)
        stats = [(sim_mtx_proto_tril.sum() * 2) / (n_prototypes * (n_prototypes - 1)), entity_to_proto.mean(dim=-1).mean(),
                 entity_to_proto.max(dim=-1).values.mean(), entity_to_proto.min(dim=-1).values.mean()]
        if other_weights is not None:
            names += ['bin_weights_mean', 'sum_weights_mean']
            stats += [(other_weights != 0).sum(dim=-1).float().mean(), other_weights.sum(dim=-1).mean()]
        return dict(zip(names, torch.stack(stats).tolist()))


def protomf_post_val_light(prototypes: torch.Tensor, entity_embeddings: torch.Tensor) -> Dict[str, float]:
    """``prototype_stats`` with the shifted similarity (sgd_alg.py:424-431, 528-535)."""
    return prototype_stats(ops.proto_sim, prototypes, entity_embeddings)


class _ProtoSide(PrototypeWrapper):
    """What UProtoMF and IProtoMF share: the prototypes, the regulariser accumulators and their bookkeeping."""

    def __init__(self, n_users: int, n_items: int, embedding_dim: int, n_prototypes: int, sim_proto_weight: float,
                 sim_batch_weight: float):
        super().__init__()
        self.n_users, self.n_items = n_users, n_items
        self.embedding_dim, self.n_prototypes = embedding_dim, n_prototypes
        self.sim_proto_weight, self.sim_batch_weight = sim_proto_weight, sim_batch_weight
        self._acc_r_proto = 0
        self._acc_r_batch = 0
        self._pending = None          # (sim matrix, proto_loss, batch_loss) of the last ProtoSimFn call

    def _init_prototypes(self):
        self.prototypes = nn.Parameter(torch.randn([self.n_prototypes, self.embedding_dim]) * .1 / self.embedding_dim, requires_grad=True)

    def _sim(self, table: torch.Tensor, idxs: torch.Tensor) -> torch.Tensor:
        if not idxs.is_cuda:
            raise RuntimeError(f'{self.name} (HIP engine) needs CUDA(HIP) index tensors')
        if not torch.is_grad_enabled():
            return ops.proto_sim(table, idxs, self.prototypes)
        sim, proto_loss, batch_loss = ops.ProtoSimFn.apply(table, idxs, self.prototypes)
        self._pending = (sim, proto_loss, batch_loss)
        return sim

    def compute_reg_losses(self, sim_mtx):
        """sgd_alg.py:394-399 / 505-510. The two minima were taken by the kernel that produced ``sim_mtx``; a similarity matrix from
        anywhere else is an error (there is no torch path)."""
        if self._pending is None or self._pending[0] is not sim_mtx:
            raise RuntimeError(f'{self.name}.compute_reg_losses needs the similarity matrix of the last get_*_representations call '
                               f'made with gradients enabled')
        _, proto_loss, batch_loss = self._pending
        self._pending = None
        self._acc_r_proto += proto_loss
        self._acc_r_batch += batch_loss

    def get_and_reset_other_loss(self) -> Dict:
        acc_r_proto, acc_r_batch = self._acc_r_proto, self._acc_r_batch
        self._acc_r_proto = self._acc_r_batch = 0
        proto_loss = self.sim_proto_weight * acc_r_proto
        batch_loss = self.sim_batch_weight * acc_r_batch
        return {'reg_loss': proto_loss + batch_loss, 'proto_loss': proto_loss, 'batch_loss': batch_loss}

    def combine_user_item_representations(self, u_repr, i_repr):
        return ops.score(u_repr, i_repr)


class UProtoMF(_ProtoSide):
    """algorithms/sgd_alg.py:332-431 — user prototypes."""

    def __init__(self, n_users: int, n_items: int, embedding_dim: int = 100, n_prototypes: int = 20, sim_proto_weight: float = 1.,
                 sim_batch_weight: float = 1.):
        super().__init__(n_users, n_items, embedding_dim, n_prototypes, sim_proto_weight, sim_batch_weight)
        self.user_embed = nn.Embedding(self.n_users, self.embedding_dim)
        self.item_embed = nn.Embedding(self.n_items, self.n_prototypes)
        self._init_prototypes()
        self.user_embed.apply(general_weight_init)
        self.item_embed.apply(general_weight_init)
        self.name = 'UProtoMF'

    def forward(self, u_idxs, i_idxs):
        u_repr = self.get_user_representations(u_idxs)
        i_repr = self.get_item_representations(i_idxs)
        dots = self.combine_user_item_representations(u_repr, i_repr)
        self.compute_reg_losses(u_repr)
        return dots

    def get_user_representations(self, u_idxs):
        return self._sim(self.user_embed.weight, u_idxs)                       # [batch_size, n_prototypes]

    def get_item_representations(self, i_idxs):
        return ops.LookupFn.apply(self.item_embed.weight, i_idxs)

    def get_user_representations_pre_tune(self, u_idxs):
        return self.get_user_representations(u_idxs)

    def get_user_representations_post_tune(self, u_repr):
        return u_repr

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        return UProtoMF(dataset.n_users, dataset.n_items, conf['embedding_dim'], conf['n_prototypes'], conf['sim_proto_weight'],
                        conf['sim_batch_weight'])

    def post_val(self, curr_epoch: int):
        return protomf_post_val_light(self.prototypes, self.user_embed.weight)


class IProtoMF(_ProtoSide):
    """algorithms/sgd_alg.py:434-535 — item prototypes."""

    def __init__(self, n_users: int, n_items: int, embedding_dim: int = 100, n_prototypes: int = 20, sim_proto_weight: float = 1.,
                 sim_batch_weight: float = 1.):
        super().__init__(n_users, n_items, embedding_dim, n_prototypes, sim_proto_weight, sim_batch_weight)
        self.user_embed = nn.Embedding(self.n_users, self.n_prototypes)
        self.item_embed = nn.Embedding(self.n_items, self.embedding_dim)
        self._init_prototypes()
        self.user_embed.apply(general_weight_init)
        self.item_embed.apply(general_weight_init)
        self.name = 'IProtoMF'

    def forward(self, u_idxs, i_idxs):
        u_repr = self.get_user_representations(u_idxs)
        i_repr = self.get_item_representations(i_idxs)
        dots = self.combine_user_item_representations(u_repr, i_repr)
        self.compute_reg_losses(i_repr)
        return dots

    def get_user_representations(self, u_idxs):
        return ops.LookupFn.apply(self.user_embed.weight, u_idxs)

    def get_item_representations(self, i_idxs):
        return self._sim(self.item_embed.weight, i_idxs)                       # [*i_idxs.shape, n_prototypes]

    def get_item_representations_pre_tune(self, i_idxs):
        return self.get_item_representations(i_idxs)

    def get_item_representations_post_tune(self, i_repr):
        return i_repr

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        return IProtoMF(dataset.n_users, dataset.n_items, conf['embedding_dim'], conf['n_prototypes'], conf['sim_proto_weight'],
                        conf['sim_batch_weight'])

    def post_val(self, curr_epoch: int):
        return protomf_post_val_light(self.prototypes, self.item_embed.weight)


class UIProtoMF(PrototypeWrapper):
    """algorithms/sgd_alg.py:538-640 — user and item prototypes; each side is also projected into the other side's prototype space."""

    def __init__(self, n_users: int, n_items: int, embedding_dim: int = 100, u_n_prototypes: int = 20, i_n_prototypes: int = 20,
                 u_sim_proto_weight: float = 1., u_sim_batch_weight: float = 1., i_sim_proto_weight: float = 1.,
                 i_sim_batch_weight: float = 1.):
        super().__init__()
        self.n_users, self.n_items, self.embedding_dim = n_users, n_items, embedding_dim
        self.uprotomf = UProtoMF(n_users, n_items, embedding_dim, u_n_prototypes, u_sim_proto_weight, u_sim_batch_weight)
        self.iprotomf = IProtoMF(n_users, n_items, embedding_dim, i_n_prototypes, i_sim_proto_weight, i_sim_batch_weight)
        self.u_to_i_proj = nn.Linear(self.embedding_dim, i_n_prototypes, bias=False)     # UProtoMF -> IProtoMF
        self.i_to_u_proj = nn.Linear(self.embedding_dim, u_n_prototypes, bias=False)     # IProtoMF -> UProtoMF
        self.u_to_i_proj.apply(general_weight_init)
        self.i_to_u_proj.apply(general_weight_init)
        # deleting unused parameters
        del self.uprotomf.item_embed
        del self.iprotomf.user_embed
        self.name = 'UIProtoMF'

    def get_user_representations(self, u_idxs):
        u_sim_mtx = self.uprotomf.get_user_representations(u_idxs)
        u_proj = ops.GatherLinearFn.apply(self.uprotomf.user_embed.weight, u_idxs, self.u_to_i_proj.weight)
        return u_sim_mtx, u_proj

    def get_item_representations(self, i_idxs):
        i_sim_mtx = self.iprotomf.get_item_representations(i_idxs)
        i_proj = ops.GatherLinearFn.apply(self.iprotomf.item_embed.weight, i_idxs, self.i_to_u_proj.weight)
        return i_sim_mtx, i_proj

    def combine_user_item_representations(self, u_repr, i_repr):
        # u_sim . i_proj + u_proj . i_sim (sgd_alg.py:590-592) as ONE product over the concatenated widths
        u_sim_mtx, u_proj = u_repr
        i_sim_mtx, i_proj = i_repr
        return ops.score(torch.cat([u_sim_mtx, u_proj], dim=-1), torch.cat([i_proj, i_sim_mtx], dim=-1))

    def get_item_representations_pre_tune(self, i_idxs):
        return self.get_item_representations(i_idxs)

    def get_item_representations_post_tune(self, i_repr):
        return i_repr

    def get_user_representations_pre_tune(self, u_idxs):
        return self.get_user_representations(u_idxs)

    def get_user_representations_post_tune(self, u_repr):
        return u_repr

    def forward(self, u_idxs, i_idxs):
        u_repr = self.get_user_representations(u_idxs)
        i_repr = self.get_item_representations(i_idxs)
        dots = self.combine_user_item_representations(u_repr, i_repr)
        self.uprotomf.compute_reg_losses(u_repr[0])
        self.iprotomf.compute_reg_losses(i_repr[0])
        return dots

    def get_and_reset_other_loss(self) -> Dict:
        u_reg = {'user_' + k: v for k, v in self.uprotomf.get_and_reset_other_loss().items()}
        i_reg = {'item_' + k: v for k, v in self.iprotomf.get_and_reset_other_loss().items()}
        return {'reg_loss': u_reg.pop('user_reg_loss') + i_reg.pop('item_reg_loss'), **u_reg, **i_reg}

    def post_val(self, curr_epoch: int):
        uprotomf_post_val = {'user_' + k: v for k, v in self.uprotomf.post_val(curr_epoch).items()}
        iprotomf_post_val = {'item_' + k: v for k, v in self.iprotomf.post_val(curr_epoch).items()}
        return {**uprotomf_post_val, **iprotomf_post_val}

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        return UIProtoMF(dataset.n_users, dataset.n_items, conf['embedding_dim'], conf['u_n_prototypes'], conf['i_n_prototypes'],
                         conf['u_sim_proto_weight'], conf['u_sim_batch_weight'], conf['i_sim_proto_weight'], conf['i_sim_batch_weight'])
