"""LightGCN (He et al., SIGIR 2020; registry name ``lightgcn``) on the engine's kernels — a sibling model of SGDMatrixFactorization. The
reference has no graph model that is trained; this one is not a port.

It is matrix factorisation whose two embedding tables pass through a fixed linear operator before the lookup. With ``E0`` the user table
stacked on the item table and ``A^ = D^-1/2 A D^-1/2`` the normalised adjacency of the bipartite graph of the training interactions, the
representations are the rows of ``E = (1 / (L + 1)) sum_{k=0..L} A^^k E0`` (``ops.LightGCNPropagateFn``: L launches of
``sbr_graph_propagate_f32`` over the resident CSR matrix and its cached transpose, fixed order, no atomics; the backward pass is the same
computation on the gradient). The lookups (``ops.LookupFn``) and scorers (``ops.ScoreDotFn``, ``ops.ScoreAllFn``) are
SGDMatrixFactorization's, and so are the state_dict keys, ``user_embeddings.weight`` and ``item_embeddings.weight``: an ``mf`` checkpoint
without biases loads. ``n_layers = 0`` is plain matrix factorisation, bit for bit.

A training step propagates once and looks both sides up in the result. In ``eval()`` mode without gradients the propagated table is
computed once and kept: full-catalogue evaluation costs one propagation, not one per user chunk. The table is dropped by ``train()``, by
``load_state_dict`` and whenever the version counter or the storage of either embedding table differs from the one it was computed
from. ``FusedOptimizer`` writes parameters through raw pointers, which no version counter sees, so it calls ``drop_propagated()`` itself on
every step; whoever else writes into the tables' storage behind autograd's back calls it too.

Deliberate differences from the paper: the separate L2 term on the batch's ego embeddings is left out (weight decay comes from the
optimizer, as for every other model here); no edge or message dropout; the graph is 0/1 (a matrix with values is refused).
"""
from __future__ import annotations

import torch
from torch import nn

from . import ops
from .features import DeviceCSR
from .sbnet import SGDBasedRecommenderAlgorithm, general_weight_init


class LightGCN(SGDBasedRecommenderAlgorithm):
    """``train_matrix``: the users x items training interactions (anything ``scipy.sparse.csr_matrix`` takes), 0/1."""

    def __init__(self, n_users: int, n_items: int, train_matrix, embedding_dim: int = 64, n_layers: int = 3):
        super().__init__()
        if not 1 <= embedding_dim <= ops.GRAPH_MAX_D:
            raise ValueError(f'LightGCN: embedding_dim={embedding_dim} outside [1, {ops.GRAPH_MAX_D}]')
        if n_layers < 0:
            raise ValueError(f'LightGCN: n_layers={n_layers} is negative')
        self.n_users, self.n_items, self.embedding_dim, self.n_layers = n_users, n_items, embedding_dim, int(n_layers)
        self.user_embeddings = nn.Embedding(n_users, embedding_dim)
        self.item_embeddings = nn.Embedding(n_items, embedding_dim)
        self.apply(general_weight_init)
        if train_matrix is None and self.n_layers > 0:
            raise ValueError(f'LightGCN: n_layers={n_layers} needs the training matrix')
        # non-persistent buffers: moves with .to(), stays out of the state_dict. Without layers there is nothing to propagate over, and
        # a model built on this one (DirectAU) may then come without a matrix
        self._graph = None if train_matrix is None else DeviceCSR(train_matrix)
        if self._graph is not None and tuple(self._graph.shape) != (n_users, n_items):
            raise ValueError(f'LightGCN: the training matrix is {tuple(self._graph.shape)}, not [{n_users}, {n_items}]')
        if self._graph is not None and self._graph.data is not None:
            raise ValueError('LightGCN: the normalised adjacency is stated for 0/1 interaction data; this matrix has values')
        self._propagated = None                                   # (key, user table, item table) of eval() mode
        self.name = 'LightGCN'

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        return LightGCN(dataset.n_users, dataset.n_items, dataset.user_sampling_matrix_train, embedding_dim=conf.get('embedding_dim', 64),
                        n_layers=conf.get('n_layers', 3))

    # ---- the propagated tables -------------------------------------------------------------------------------------------------------
    def _propagate(self):
        """-> (user table [n_users, D], item table [n_items, D]): views of one propagated joint table, on the autograd tape"""
        uw, iw = self.user_embeddings.weight, self.item_embeddings.weight
        if not uw.is_cuda:
            raise RuntimeError('LightGCN (HIP engine) needs its parameters on a CUDA(HIP) device')
        if self.n_layers == 0:
            return uw, iw
        e = ops.LightGCNPropagateFn.apply(self._graph, torch.cat([uw, iw], 0), self.n_layers)
        return e[:self.n_users], e[self.n_users:]

    def _cache_key(self):
        uw, iw = self.user_embeddings.weight, self.item_embeddings.weight
        return uw._version, iw._version, uw.data_ptr(), iw.data_ptr()

    def _tables(self):
        if self.training or torch.is_grad_enabled():
            return self._propagate()
        key = self._cache_key()
        if self._propagated is None or self._propagated[0] != key:
            u, i = self._propagate()
            self._propagated = (key, u.detach(), i.detach())
        return self._propagated[1:]

    def drop_propagated(self):
        self._propagated = None

    def train(self, mode: bool = True):
        self._propagated = None
        return super().train(mode)

    def load_state_dict(self, *args, **kwargs):
        self._propagated = None
        return super().load_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self._propagated = None
        return super()._apply(fn, *args, **kwargs)

    # ---- the reference's surface -----------------------------------------------------------------------------------------------------
    def get_user_representations(self, u_idxs):
        return ops.LookupFn.apply(self._tables()[0], u_idxs)

    def get_item_representations(self, i_idxs):
        return ops.LookupFn.apply(self._tables()[1], i_idxs)

    def combine_user_item_representations(self, u_repr, i_repr):
        if i_repr.ndim == 3 and i_repr.shape[0] == 1:             # [1, I, D]: broadcast over users, as in SGDMatrixFactorization
            i_repr = i_repr[0]
        return (ops.ScoreDotFn if i_repr.ndim == 3 else ops.ScoreAllFn).apply(u_repr, i_repr)

    def forward(self, u_idxs, i_idxs):
        if not i_idxs.is_cuda:
            raise RuntimeError('LightGCN (HIP engine) needs CUDA(HIP) index tensors')
        users, items = self._tables()                             # one propagation for both sides
        u_repr = ops.LookupFn.apply(users, u_idxs)
        i_repr = ops.LookupFn.apply(items, i_idxs)
        return self.combine_user_item_representations(u_repr, i_repr)
