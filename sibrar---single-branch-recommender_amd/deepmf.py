"""DeepMatrixFactorization (algorithms/sgd_alg.py:1141-1276; Xue et al., IJCAI 2017; registry name ``dmf``) on the engine's kernels — a
sibling model of SingleBranchNet. Both towers are ``PolyLinear`` stacks over RAW interaction rows: the user tower reads a user's row of
the user x item matrix, the item tower an item's row of its transpose. Nothing is densified: layer 0 of each tower multiplies the
resident CSR matrix with the column-major weight (``ops.SparseLinearActFn`` over ``sbr_csr_project_fwd`` / ``_bwd_gather``), the
remaining layers are ``ops.LinearActFn``, and the scorer is the fused cosine with a floor (``ops.ScoreCosFn``; equation 13 of the paper).
state_dict keys as in the reference: ``{user,item}_nn.layers.linear_{i}.{weight,bias}``.
"""
from __future__ import annotations

import os
import re
from typing import List, Union

import torch
from torch import nn

from . import ops
from .features import DeviceCSR
from .polylinear import PolyLinear
from .sbnet import SGDBasedRecommenderAlgorithm, general_weight_init

REPR_EPS = 1e-8                   # norm.clamp(min=1e-8), sgd_alg.py:1213, 1219


class DeepMatrixFactorization(SGDBasedRecommenderAlgorithm):
    """algorithms/sgd_alg.py:1141-1242."""

    def __init__(self, dataset, u_mid_layers: Union[List[int], int], i_mid_layers: Union[List[int], int], final_dimension: int,
                 mu: float = 1.e-6, normalize_interactions: bool = False, normalize_representations: bool = False,
                 use_output_activation_fn: bool = False):
        super().__init__()
        self.dataset = dataset
        self.normalize_interactions = normalize_interactions
        self.normalize_representations = normalize_representations
        self.mu = mu
        self.final_dimension = final_dimension

        if isinstance(u_mid_layers, int):
            u_mid_layers = [u_mid_layers]
        if isinstance(i_mid_layers, int):
            i_mid_layers = [i_mid_layers]
        self.u_layers = [self.dataset.n_items] + list(u_mid_layers) + [self.final_dimension]
        self.i_layers = [self.dataset.n_users] + list(i_mid_layers) + [self.final_dimension]

        # output activation as done in the original paper
        output_fn = nn.ReLU() if use_output_activation_fn else None
        self.user_nn = PolyLinear(self.u_layers, activation_fn=nn.ReLU(), output_fn=output_fn)
        self.item_nn = PolyLinear(self.i_layers, activation_fn=nn.ReLU(), output_fn=output_fn)
        self.user_nn.apply(general_weight_init)
        self.item_nn.apply(general_weight_init)
        for tower in (self.user_nn, self.item_nn):
            # layer 0 keeps its state_dict shape [out, n_cols] but is stored column-major: every stored entry of an interaction row
            # then reads one contiguous weight row (FeatureEmbedding keeps its CSR projector the same way)
            lin = tower.layers.linear_0
            lin.weight = nn.Parameter(lin.weight.data.t().contiguous().t())

        # get_user_interaction_vectors / get_item_interaction_vectors of the dataset (data/dataset.py:260-273), resident; with
        # normalize_interactions the per-row scale 1 / max(||row||, 1e-8) is folded into the stored values once
        self._user_rows = DeviceCSR(dataset.user_sampling_matrix_train, l2_normalize_rows=normalize_interactions)
        self._item_rows = DeviceCSR(dataset.item_sampling_matrix_train, l2_normalize_rows=normalize_interactions)
        self.name = 'DeepMatrixFactorization'

    @staticmethod
    def build_from_conf(conf: dict, train_dataset):
        return DeepMatrixFactorization(dataset=train_dataset, u_mid_layers=conf.get('u_mid_layers', []),
                                       i_mid_layers=conf.get('i_mid_layers', []), final_dimension=conf['final_dimension'],
                                       mu=conf.get('mu', 1e-6), normalize_interactions=conf.get('normalize_interactions', False),
                                       normalize_representations=conf.get('normalize_representations', False),
                                       use_output_activation_fn=conf.get('use_output_activation_fn', False))

    def _tower(self, tower: PolyLinear, rows: DeviceCSR, idxs: torch.Tensor) -> torch.Tensor:
        if not idxs.is_cuda:
            raise RuntimeError('DeepMatrixFactorization (HIP engine) needs CUDA(HIP) index tensors')
        plan = tower.layer_plan()
        lin, _, act = plan[0]
        x = ops.SparseLinearActFn.apply(rows, idxs.reshape(-1), lin.weight, lin.bias, act)
        for lin, _, act in plan[1:]:
            x = ops.LinearActFn.apply(x, lin.weight, lin.bias, act)
        if self.normalize_representations:
            x = ops.L2NormalizeFn.apply(x, REPR_EPS)
        return x.reshape(*idxs.shape, x.shape[-1])

    def get_user_representations(self, u_idxs: torch.Tensor) -> torch.Tensor:
        return self._tower(self.user_nn, self._user_rows, u_idxs)

    def get_item_representations(self, i_idxs: torch.Tensor) -> torch.Tensor:
        return self._tower(self.item_nn, self._item_rows, i_idxs)

    def combine_user_item_representations(self, u_repr: torch.Tensor, i_repr: torch.Tensor) -> torch.Tensor:
        if i_repr.ndim == 2:
            return ops.score_cos_all(u_repr, i_repr, self.mu)
        return ops.ScoreCosFn.apply(u_repr, i_repr, self.mu)

    def fused_score_transform(self):
        """``(items_fn, users_fn, finish_fn)`` for the fused full-catalogue scorers (``evaluation._score_split``), which compute plain
        dot products: both sides are row-normalised with eps 1e-8 first, so the dot product IS the cosine, and the values of every
        list are floored at ``mu`` afterwards (empty slots, ``idx < 0``, stay ``-inf``). This is exact because the floor is monotone: the
        top-k of the floored scores is the top-k of the raw cosines with the values floored afterwards. The two can differ only in the
        ORDER of entries tied at the floor, which the reference leaves to ``torch.topk``, i.e. unspecified."""
        mu = float(self.mu)

        def finish(val, idx):
            return torch.where((idx >= 0) & (val < mu), torch.full_like(val, mu), val), idx

        return ops.l2_normalize_rows, ops.l2_normalize_rows, finish

    def load_model_from_path(self, path: str):
        """sgd_alg.py:1244-1276, with the legacy key layout of earlier DMF checkpoints."""
        path = os.path.join(path, 'model.pth')
        self.load_state_dict(self.map_legacy_state_dict(torch.load(path, weights_only=True)))
        print('Model Loaded')

    @staticmethod
    def map_legacy_state_dict(state_dict: dict) -> dict:
        # earlier DMF versions also saved the user and item interactions in the model file
        if 'user_vectors.weight' not in state_dict:
            return state_dict
        state_dict = dict(state_dict)
        # not needed: the interactions come from the dataset
        state_dict.pop('user_vectors.weight')
        state_dict.pop('item_vectors.weight')

        def to_new_key(k):
            # old keys: user_nn.0.weight, user_nn.2.weight -> new keys: user_nn.layers.linear_0.weight, user_nn.layers.linear_1.weight
            match_obj = re.match(r'^(\w+)\.(\d+)\.(\w+)$', k)
            if match_obj is not None:
                old_layer_nr = int(match_obj[2])
                if old_layer_nr % 2 != 0:
                    raise ValueError('did not expect an odd layer number for old-version parameter names')
                return f'{match_obj[1]}.layers.linear_{int(old_layer_nr / 2)}.{match_obj[3]}'
            return k

        return {to_new_key(k): v for k, v in state_dict.items()}
