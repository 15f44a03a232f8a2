"""NGCF (Wang et al., "Neural Graph Collaborative Filtering", SIGIR 2019; registry name ``ngcf``) on the engine's kernels — the model
LightGCN simplifies, and the first graph model here whose layers have parameters. The reference has no such model; this is not a port.

With ``E(0)`` the user table stacked on the item table and ``A^ = D^-1/2 A D^-1/2`` LightGCN's operator, layer l computes
    S    = A^ E(l-1)
    E(l) = dropout( LeakyReLU( (S + E(l-1)) W1(l) + (S * E(l-1)) W2(l) + b(l) ) )
and the representations are the rows of ``[E(0) | normalize(E(1)) | ... | normalize(E(L))]`` (row-wise L2), ``embedding_dim +
sum(layer_sizes)`` wide. One launch per layer (``ops.NGCFPropagateFn`` on ``sbr_ngcf_layer_fwd``, csrc/ngcf.hip): a workgroup gathers S
for 64 rows into LDS, runs both products from there and writes the normalised rows into the layer's column slice of the representation;
S, S + E and S * E never reach memory. The backward pass is one ``sbr_ngcf_layer_bwd`` and one ``sbr_graph_propagate_f32`` per layer;
the weight gradients are per-workgroup partials folded in workgroup order, so a training step is valid in deterministic mode.

``NGCF`` is ``LightGCN`` with ``_propagate`` overridden: the 0/1 graph checks, the eval-mode cache of the propagated table (one
propagation, L launches, for a whole full-catalogue evaluation), ``drop_propagated`` and the ``train`` / ``load_state_dict`` / ``_apply``
hooks, the lookups and the scorers are inherited; the cache key also covers the layer weights. The two tables keep ``mf``'s state_dict
keys (an ``mf`` checkpoint without biases loads with ``strict=False``); layer l (0-based) adds ``w_gc.l`` (W1), ``w_bi.l`` (W2), both
[in, out], Xavier-uniform as in the paper, and ``b.l`` [out], zeros. ``layer_sizes=()`` is plain ``mf``, bit for bit, and launches none of
the new entries. Message dropout applies in training mode only: the mask is Philox4x32-10 of (seed, layer, row, column) with the seed
drawn per step from torch's CPU generator, so ``reproducible(seed)`` fixes a run; ``eval()`` draws nothing.

Deliberate differences from the paper: one bias per layer (the authors' two are added to the same sum, so they are redundant); no node
(edge) dropout; the separate L2 term on the batch's embeddings is left out (weight decay is the optimizer's, as for every model here);
the layers are L2-normalised before they are concatenated, as in the authors' code and RecBole, not as in the paper's equation 9.
"""
from __future__ import annotations

import torch
from torch import nn

from . import ops
from .lightgcn import LightGCN


class NGCF(LightGCN):
    """``train_matrix``: the users x items training interactions, 0/1; ``layer_sizes``: the output width of every layer (each in
    [1, 128], like ``embedding_dim``); ``message_dropout``: the rate p in [0, 1); ``leaky_slope`` in (0, 1]."""

    def __init__(self, n_users: int, n_items: int, train_matrix, embedding_dim: int = 64, layer_sizes=(64, 64, 64),
                 message_dropout: float = 0.1, leaky_slope: float = 0.2):
        layer_sizes = tuple(int(s) for s in layer_sizes)
        cap = ops.NGCF_MAX_WIDTH
        if layer_sizes and not all(1 <= d <= cap for d in (embedding_dim,) + layer_sizes):
            raise ValueError(f'NGCF: embedding_dim={embedding_dim} and layer_sizes={layer_sizes} must lie in [1, {cap}]')
        if not 0 <= message_dropout < 1:
            raise ValueError(f'NGCF: message_dropout={message_dropout} outside [0, 1)')
        if not 0 < leaky_slope <= 1:
            raise ValueError(f'NGCF: leaky_slope={leaky_slope} outside (0, 1]')
        super().__init__(n_users, n_items, train_matrix, embedding_dim=embedding_dim, n_layers=len(layer_sizes))
        self.layer_sizes, self.message_dropout, self.leaky_slope = layer_sizes, float(message_dropout), float(leaky_slope)
        widths = (embedding_dim,) + layer_sizes
        self.w_gc = nn.ParameterList(nn.Parameter(torch.empty(a, b)) for a, b in zip(widths[:-1], widths[1:]))
        self.w_bi = nn.ParameterList(nn.Parameter(torch.empty(a, b)) for a, b in zip(widths[:-1], widths[1:]))
        self.b = nn.ParameterList(nn.Parameter(torch.zeros(b)) for b in widths[1:])
        for w in list(self.w_gc) + list(self.w_bi):
            nn.init.xavier_uniform_(w)
        self.repr_dim = sum(widths)
        self.name = 'NGCF'

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        return NGCF(dataset.n_users, dataset.n_items, dataset.user_sampling_matrix_train, embedding_dim=conf.get('embedding_dim', 64),
                    layer_sizes=conf.get('layer_sizes', (64, 64, 64)), message_dropout=conf.get('message_dropout', 0.1),
                    leaky_slope=conf.get('leaky_slope', 0.2))

    def _layer_params(self):
        return [t for l in range(self.n_layers) for t in (self.w_gc[l], self.w_bi[l], self.b[l])]

    def _propagate(self):
        """-> (user table, item table) [., repr_dim]: views of the concatenated joint table, on the autograd tape"""
        uw, iw = self.user_embeddings.weight, self.item_embeddings.weight
        if not uw.is_cuda:
            raise RuntimeError('NGCF (HIP engine) needs its parameters on a CUDA(HIP) device')
        if self.n_layers == 0:
            return uw, iw
        p, seed = 0.0, 0
        if self.training and self.message_dropout > 0:
            p, seed = self.message_dropout, int(torch.randint(0, 1 << 62, (1,)).item())      # the CPU generator: no synchronisation
        e = ops.NGCFPropagateFn.apply(self._graph, torch.cat([uw, iw], 0), self.leaky_slope, p, seed, *self._layer_params())
        return e[:self.n_users], e[self.n_users:]

    def _cache_key(self):
        return tuple(k for t in [self.user_embeddings.weight, self.item_embeddings.weight] + self._layer_params()
                     for k in (t._version, t.data_ptr()))
