"""ECF — Explainable Collaborative Filtering (Du et al., WWW 2023) on the engine's kernels — algorithms/sgd_alg.py:891-1138, registry name
``ecf``; the last of the cluster baselines ProtoMF and ACF are compared with, behind the same plugin surface (PrototypeWrapper). An item is
affiliated to its ``top_m`` closest taste clusters, a user to the ``top_n`` clusters the items they interacted with point to.

The affiliation of either side is ONE op each way, ``ops.ClusterAffilFn`` (csrc/cluster_affil.hip): cosine logits (item side), the exact
top-k mask, the softmax mask with its straight-through gradient and the sigmoid. The interaction matrix and the tag matrix stay CSR and
resident (``features.DeviceCSR``, the tag matrix transposed): ``Y[u_idxs] @ x_tildes`` and ``tag_matrix^T @ xs`` are
``ops.csr_rows_times_dense``; nothing of size U x I, B x I or I x T is ever built. The [T, C] and [C, C] tails of the two regularisers and
the BCE of the BPR term are torch ops on the device. The regulariser values stay on the device: ``get_and_reset_other_loss`` never
synchronises.

Deviations from the reference, both listed in INTEGRATION.md: the state_dict has no ``interaction_matrix`` entry (the reference registers
the dense float32 matrix as a parameter; such an entry is accepted and dropped on loading), and ``build_from_conf`` falls back to
``dataset.user_sampling_matrix_train`` when the dataset has no ``sampling_matrix``. Equal logits at the boundary of a mask go to the
lowest cluster index (torch.topk leaves that open).
"""
from __future__ import annotations

import inspect
import os
from typing import Dict

import numpy as np
import scipy.sparse as sp
import torch
from torch import nn
from torch.nn import functional as F

from . import ops
from .features import DeviceCSR
from .protomf import PrototypeWrapper


def ecf_tag_matrix(n_items: int, item_idx, tag_idx, n_tags: int) -> sp.csr_matrix:
    """data/dataset.py:469-483 (ECFTrainRecDataset._prepare_tag_data) from the two columns of ``item_tag_idxs.csv``: the item x tag
    incidence matrix (duplicate pairs add up, as in the reference) with every tag column weighted by ``log(n_items / (freq + 1e-6))``."""
    item_idx, tag_idx = np.asarray(item_idx), np.asarray(tag_idx)
    tag_matrix = sp.csr_matrix((np.ones(len(item_idx), dtype=np.int16), (item_idx, tag_idx)), shape=(n_items, n_tags))
    tag_frequency = np.array(tag_matrix.sum(axis=0)).flatten()
    tag_weight = np.log(n_items / (tag_frequency + 1e-6))
    return sp.csr_matrix(tag_matrix @ sp.diags(tag_weight))


class ECF(PrototypeWrapper):
    """algorithms/sgd_alg.py:891-1138."""

    def __init__(self, n_users: int, n_items: int, tag_matrix: sp.csr_matrix, interaction_matrix: sp.csr_matrix,
                 embedding_dim: int = 100, n_clusters: int = 64, top_n: int = 20, top_m: int = 20, temp_masking: float = 2.,
                 temp_tags: float = 2., top_p: int = 4, lam_cf: float = 0.6, lam_ind: float = 1., lam_ts: float = 1.):
        super().__init__()
        self.n_users, self.n_items = n_users, n_items
        tag_matrix, interaction_matrix = sp.csr_matrix(tag_matrix), sp.csr_matrix(interaction_matrix)
        if tag_matrix.shape[0] != n_items or interaction_matrix.shape != (n_users, n_items):
            raise ValueError(f'ECF: tag matrix {tag_matrix.shape} / interaction matrix {interaction_matrix.shape} do not fit '
                             f'{n_users} users and {n_items} items')
        # resident CSR, never densified (the reference keeps both dense in fp32, sgd_alg.py:905-906); the tag matrix transposed: its
        # product with xs is taken per tag
        self.tag_matrix_t = DeviceCSR(sp.csr_matrix(tag_matrix.T))
        self.interaction_matrix = DeviceCSR(interaction_matrix)
        self.n_tags = int(tag_matrix.shape[1])
        self.embedding_dim, self.n_clusters = embedding_dim, n_clusters
        self.top_n, self.top_m = top_n, top_m
        self.temp_masking, self.temp_tags, self.top_p = temp_masking, temp_tags, top_p
        self.lam_cf, self.lam_ind, self.lam_ts = lam_cf, lam_ind, lam_ts
        self.user_embed = nn.Embedding(self.n_users, self.embedding_dim)
        self.item_embed = nn.Embedding(self.n_items, self.embedding_dim)
        indxs = torch.randperm(self.n_items)[:self.n_clusters]
        self.clusters = nn.Parameter(self.item_embed.weight[indxs].detach().clone(), requires_grad=True)
        self._acc_ts = 0
        self._acc_ind = 0
        self._acc_cf = 0
        # set by every item call (sgd_alg.py:930-932)
        self._x_tildes = None
        self._xs = None
        self._tag_rows = None
        self.name = 'ECF'

    # ---- the two sides -----------------------------------------------------------------------------------------------------------
    def _generate_item_representations(self):
        """sgd_alg.py:1020-1037 over the whole catalogue: caches x_tildes and xs [n_items, n_clusters]."""
        if not self.clusters.is_cuda:
            raise RuntimeError(f'{self.name} (HIP engine) needs its parameters on a CUDA(HIP) device')
        if torch.is_grad_enabled():
            self._x_tildes, self._xs = ops.ClusterAffilFn.apply(self.item_embed.weight, self.clusters, None, self.top_m, self.temp_masking)
        else:
            self._x_tildes, self._xs = ops.cluster_affil(self.item_embed.weight, self.clusters, None, self.top_m, self.temp_masking)

    def _check_idxs(self, idxs):
        if not idxs.is_cuda:
            raise RuntimeError(f'{self.name} (HIP engine) needs CUDA(HIP) index tensors')

    def get_item_representations(self, i_idxs):
        self._check_idxs(i_idxs)
        self._generate_item_representations()
        return ops.LookupFn.apply(self._xs, i_idxs), ops.LookupFn.apply(self.item_embed.weight, i_idxs)

    def get_user_representations(self, u_idxs):
        self._check_idxs(u_idxs)
        if self._x_tildes is None:
            raise RuntimeError(f'{self.name}: the user representations are built from the item logits of the current parameters — call '
                               f'get_item_representations (or get_item_representations_pre_tune) first')
        u_embed = ops.LookupFn.apply(self.user_embed.weight, u_idxs)
        a_tilde = ops.csr_rows_times_dense(self.interaction_matrix, u_idxs, self._x_tildes)             # [batch_size, n_clusters]
        if torch.is_grad_enabled():
            a_i = ops.ClusterAffilFn.apply(None, None, a_tilde, self.top_n, self.temp_masking)
        else:
            a_i = ops.cluster_affil(None, None, a_tilde, self.top_n, self.temp_masking)
        return a_i, u_embed

    def combine_user_item_representations(self, u_repr, i_repr):
        return ops.score(u_repr[0], i_repr[0])                  # a_i . x_i

    def forward(self, u_idxs, i_idxs):
        i_repr = self.get_item_representations(i_idxs)
        # NB (the reference's): item representations are generated before the user representations
        u_repr = self.get_user_representations(u_idxs)
        dots = self.combine_user_item_representations(u_repr, i_repr)
        # tag loss (the frequency weights are in the tag matrix): d_c^T = tag_matrix^T @ xs, [n_tags, n_clusters]
        if self._tag_rows is None or self._tag_rows.device != u_idxs.device:
            self._tag_rows = torch.arange(self.n_tags, device=u_idxs.device, dtype=torch.int32)
        d_c_t = ops.csr_rows_times_dense(self.tag_matrix_t, self._tag_rows, self._xs)
        log_b_c = F.log_softmax(d_c_t / self.temp_tags, dim=0)
        self._acc_ts += (-log_b_c.topk(self.top_p, dim=0).values).sum()
        # independence loss
        c_norm = F.normalize(self.clusters)
        sim_mtx = torch.clamp(c_norm @ c_norm.T, min=-1., max=1.)
        self._acc_ind += torch.diag(-F.log_softmax(sim_mtx, dim=-1)).sum()
        # BPR loss on the raw embeddings
        logits = ops.ScoreDotFn.apply(u_repr[1], i_repr[1])
        diff_logits = (logits[:, :1] - logits[:, 1:]).flatten()
        self._acc_cf += F.binary_cross_entropy_with_logits(diff_logits, torch.ones_like(diff_logits))
        return dots

    def get_item_representations_pre_tune(self, i_idxs=None):
        # i_idxs is ignored (sgd_alg.py:1047-1066)
        with torch.no_grad():
            self._generate_item_representations()
        return self._xs, self.item_embed.weight

    def get_item_representations_post_tune(self, i_repr):
        return i_repr

    def get_user_representations_pre_tune(self, u_idxs):
        with torch.no_grad():
            return self.get_user_representations(u_idxs)

    def get_user_representations_post_tune(self, u_repr):
        return u_repr

    def get_and_reset_other_loss(self) -> Dict:
        acc_ts, acc_ind, acc_cf = self._acc_ts, self._acc_ind, self._acc_cf
        self._acc_ts = self._acc_ind = self._acc_cf = 0
        cf_loss = self.lam_cf * acc_cf
        ind_loss = self.lam_ind * acc_ind
        ts_loss = self.lam_ts * acc_ts
        return {'reg_loss': ts_loss + ind_loss + cf_loss, 'cf_loss': cf_loss, 'ind_loss': ind_loss, 'ts_loss': ts_loss}

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        init_signature = inspect.signature(ECF.__init__)
        def_parameters = {k: v.default for k, v in init_signature.parameters.items() if v.default is not inspect.Parameter.empty}
        parameters = {**def_parameters, **conf}
        # the reference reads dataset.sampling_matrix (sgd_alg.py:1120), which its own dataset classes never set: fall back to the
        # training interactions they do have
        interactions = getattr(dataset, 'sampling_matrix', None)
        if interactions is None:
            interactions = dataset.user_sampling_matrix_train
        return ECF(dataset.n_users, dataset.n_items, dataset.tag_matrix, interactions, parameters['embedding_dim'],
                   parameters['n_clusters'], parameters['top_n'], parameters['top_m'], parameters['temp_masking'], parameters['temp_tags'],
                   parameters['top_p'], parameters['lam_cf'], parameters['lam_ind'], parameters['lam_ts'])

    # ---- checkpoints -----------------------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict: bool = True, **kwargs):
        """A reference checkpoint carries the dense interaction matrix as ``interaction_matrix``: accepted and dropped."""
        state_dict = {k: v for k, v in state_dict.items() if k != 'interaction_matrix'}
        return super().load_state_dict(state_dict, strict=strict, **kwargs)

    def load_model_from_path(self, path: str):
        # sgd_alg.py:1134-1138: strict=False
        state_dict = torch.load(os.path.join(path, 'model.pth'), map_location=self.clusters.device, weights_only=True)
        self.load_state_dict(state_dict, strict=False)
        print('Model Loaded')
