"""SimGCL (Yu et al., "Are Graph Augmentations Necessary?", SIGIR 2022; registry name ``simgcl``) and XSimGCL (Yu et al., "XSimGCL: Towards
Extremely Simple Graph Contrastive Learning for Recommendation", TKDE 2023; ``xsimgcl``) on the engine's kernels. The reference has no
such model; these are not ports.

Both are ``LightGCN`` whose layers are perturbed while training: ``E_k = A^ E_(k-1) + sign(.) * eps * u / |u_row|`` with ``u`` uniform in
[0, 1), the representations the mean of the layers 1 .. L (layer 0, the raw tables, is left out, as in the authors' code), trained with
the recommendation loss on the logits plus an InfoNCE term between two views of the same rows. The perturbation is made inside the
propagation launch (``ops.NoisyPropagateFn`` on ``sbr_graph_propagate_noise_f32``): the noise is a pure function of (seed, step, view,
layer, row, column), generated in the registers of the lane that owns the element, and never touches memory. The backward pass is the
linear operator alone, L launches of ``sbr_graph_propagate_f32``.

  ``XSimGCL``  one noisy propagation per step (view 0). The logits come from its mean; the contrast is between the mean and the kept
               layer ``keep_layer`` (the paper's l*).
  ``SimGCL``   one clean propagation for the logits, two noisy ones (views 1 and 2) for the contrast.

The model counts its training forwards; the count is the ``step`` of the noise, so every step draws afresh and a run is reproducible
from ``seed`` alone. The contrast is taken over the DISTINCT users of the batch and, separately, over its DISTINCT positive items
(``torch.unique``: one synchronisation with the host per step), both views L2-normalised: ``ops.InfoNCEFn`` with G = 1, N = the number of
distinct rows, ``mean=True``. In training mode ``forward`` returns the logits and keeps ``cl_weight * (cl_users + cl_items)`` for
``get_and_reset_other_loss`` as ``reg_loss``, with the two terms detached beside it as ``cl_u`` and ``cl_i``. ``cl_weight = 0`` computes
the terms as figures, without gradient. In deterministic mode (``ops.set_deterministic``) a contrast over at most
``ops.infonce_max_n()`` = 176 distinct rows takes InfoNCE's one-workgroup entry, which has a fixed order; over more rows it is the
GEMM route, whose forward has no deterministic form and raises there.

Without noise — ``eval()`` mode, or any pass outside a training forward — the table is the ``eps = 0`` propagation with the layer-1..L
mean. That is NOT LightGCN's table, which includes layer 0. It is cached and dropped by LightGCN's rules (``_propagate`` is overridden,
nothing else); scores are dot products, so the fused scorers are reached as for ``lightgcn``. The state_dict keys are ``mf``'s:
``mf`` checkpoints without biases and ``lightgcn`` checkpoints load.

Deliberate differences from the papers: ``ops.InfoNCEFn`` is the symmetric loss (both retrieval directions) where the authors use one
direction, so it is multiplied by 1/2; the papers' L2 term on the batch's embeddings is the optimizer's weight decay; the noise is
counter-based (Philox4x32-10 keyed by ``seed``), not the device generator's stream; the graph is 0/1.
"""
from __future__ import annotations

import torch

from . import ops
from .lightgcn import LightGCN


class _NoisyLightGCN(LightGCN):
    """what SimGCL and XSimGCL share: the hyperparameters, the clean layer-1..L table, the step count and the contrast term"""

    def __init__(self, n_users: int, n_items: int, train_matrix, embedding_dim: int, n_layers: int, eps: float, cl_weight: float, tau: float,
                 seed: int, keep_layer=None):
        who = type(self).__name__
        if n_layers < 1:
            raise ValueError(f'{who}: n_layers={n_layers}: with no layer there is nothing to perturb')
        if not 0 <= eps < float('inf'):
            raise ValueError(f'{who}: eps={eps} must be finite and not negative')
        if not tau > 0:
            raise ValueError(f'{who}: tau={tau} must be positive')
        if not cl_weight >= 0:
            raise ValueError(f'{who}: cl_weight={cl_weight} is negative')
        if n_layers >= ops.GRAPH_NOISE_MAX_LAYERS:
            raise ValueError(f'{who}: n_layers={n_layers}: the noise streams are numbered for fewer than {ops.GRAPH_NOISE_MAX_LAYERS} layers')
        if keep_layer is not None and not 1 <= keep_layer <= n_layers:
            raise ValueError(f'{who}: keep_layer={keep_layer} outside [1, {n_layers}]')
        if int(seed) != seed or not 0 <= seed < 1 << 64:
            raise ValueError(f'{who}: seed={seed!r} must be an integer in [0, 2^64)')
        super().__init__(n_users, n_items, train_matrix, embedding_dim=embedding_dim, n_layers=n_layers)
        self.eps, self.cl_weight, self.tau, self.seed = float(eps), float(cl_weight), float(tau), int(seed)
        self.keep_layer = None if keep_layer is None else int(keep_layer)
        self.step = 0                                             # training forwards so far: the noise's step
        self._contrast = None                                     # (weighted term, cl_u, cl_i) of the last training forward
        self.name = who

    def _joint(self):
        uw, iw = self.user_embeddings.weight, self.item_embeddings.weight
        if not uw.is_cuda:
            raise RuntimeError(f'{self.name} (HIP engine) needs its parameters on a CUDA(HIP) device')
        return torch.cat([uw, iw], 0)

    def _noisy(self, e0, step, view, keep_layer=None):
        return ops.NoisyPropagateFn.apply(self._graph, e0, self.n_layers, self.eps, self.seed, step, view, keep_layer)

    def _propagate(self):
        """-> (user table, item table): the clean (eps = 0) mean of the layers 1 .. L, on the autograd tape"""
        e, _ = ops.NoisyPropagateFn.apply(self._graph, self._joint(), self.n_layers, 0.0, self.seed, 0, 0, None)
        return e[:self.n_users], e[self.n_users:]

    def _views(self, e0, step):
        """-> (the joint table of the logits, the two joint tables of the contrast)"""
        raise NotImplementedError

    def _info_nce(self, a, b, rows):
        va = ops.L2NormalizeFn.apply(ops.LookupFn.apply(a, rows))
        vb = ops.L2NormalizeFn.apply(ops.LookupFn.apply(b, rows))
        # deterministic mode: the GEMM route's loss is an arrival-order sum and is refused there, so up to infonce_max_n() distinct rows
        # take the one-workgroup entry, which has a fixed order; more rows than that have no deterministic form
        n = rows.numel()
        gemm = False if ops.is_deterministic() and n <= ops.infonce_max_n() else None
        return ops.InfoNCEFn.apply(torch.stack([va, vb], 1), self.tau, True, 1, n, gemm) * 0.5

    def forward(self, u_idxs, i_idxs):
        if not self.training:
            return super().forward(u_idxs, i_idxs)
        if not i_idxs.is_cuda:
            raise RuntimeError(f'{self.name} (HIP engine) needs CUDA(HIP) index tensors')
        if i_idxs.dim() != 2 or u_idxs.dim() != 1:
            raise ValueError(f'{self.name}: a training batch is u_idxs [B] and i_idxs [B, 1 + N] with the positive in column 0, got '
                             f'{tuple(u_idxs.shape)} and {tuple(i_idxs.shape)}')
        step, self.step = self.step, self.step + 1
        table, a, b = self._views(self._joint(), step)
        u_repr = ops.LookupFn.apply(table[:self.n_users], u_idxs)
        i_repr = ops.LookupFn.apply(table[self.n_users:], i_idxs)
        users = torch.unique(u_idxs)                              # the one synchronisation of a step: the counts size the contrast
        items = torch.unique(i_idxs[:, 0]) + self.n_users
        with torch.set_grad_enabled(self.cl_weight > 0 and torch.is_grad_enabled()):  # cl_weight = 0: the terms are figures, not objectives
            cl_u, cl_i = self._info_nce(a, b, users), self._info_nce(a, b, items)
            self._contrast = (self.cl_weight * (cl_u + cl_i), cl_u.detach(), cl_i.detach())
        return self.combine_user_item_representations(u_repr, i_repr)

    def get_and_reset_other_loss(self):
        kept, self._contrast = self._contrast, None
        if kept is None:
            zero = torch.zeros((), device=self.device)
            kept = (zero, zero, zero)
        return {'reg_loss': kept[0], 'cl_u': kept[1], 'cl_i': kept[2]}


class SimGCL(_NoisyLightGCN):
    """``train_matrix``: the users x items training interactions, 0/1; ``eps``: the length of a row's perturbation; ``cl_weight``: the
    paper's lambda; ``tau``: the temperature of the contrast; ``seed``: the key of the noise."""

    def __init__(self, n_users: int, n_items: int, train_matrix, embedding_dim: int = 64, n_layers: int = 3, eps: float = 0.1,
                 cl_weight: float = 0.2, tau: float = 0.2, seed: int = 0):
        super().__init__(n_users, n_items, train_matrix, embedding_dim, n_layers, eps, cl_weight, tau, seed)

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        return SimGCL(dataset.n_users, dataset.n_items, dataset.user_sampling_matrix_train, embedding_dim=conf.get('embedding_dim', 64),
                      n_layers=conf.get('n_layers', 3), eps=conf.get('eps', 0.1), cl_weight=conf.get('cl_weight', 0.2),
                      tau=conf.get('tau', 0.2), seed=conf.get('seed', 0))

    def _views(self, e0, step):
        clean, _ = ops.NoisyPropagateFn.apply(self._graph, e0, self.n_layers, 0.0, self.seed, step, 0, None)
        return clean, self._noisy(e0, step, 1)[0], self._noisy(e0, step, 2)[0]


class XSimGCL(_NoisyLightGCN):
    """``keep_layer``: the layer the final representation is contrasted with (the paper's l*), in [1, n_layers]; the rest as ``SimGCL``."""

    def __init__(self, n_users: int, n_items: int, train_matrix, embedding_dim: int = 64, n_layers: int = 2, eps: float = 0.1,
                 cl_weight: float = 0.2, tau: float = 0.2, seed: int = 0, keep_layer: int = 1):
        if keep_layer is None:
            raise ValueError('XSimGCL: keep_layer is needed: the contrast is between the mean and that layer')
        super().__init__(n_users, n_items, train_matrix, embedding_dim, n_layers, eps, cl_weight, tau, seed, keep_layer)

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        return XSimGCL(dataset.n_users, dataset.n_items, dataset.user_sampling_matrix_train, embedding_dim=conf.get('embedding_dim', 64),
                       n_layers=conf.get('n_layers', 2), eps=conf.get('eps', 0.1), cl_weight=conf.get('cl_weight', 0.2),
                       tau=conf.get('tau', 0.2), seed=conf.get('seed', 0), keep_layer=conf.get('keep_layer', 1))

    def _views(self, e0, step):
        mean, kept = self._noisy(e0, step, 0, self.keep_layer)
        return mean, mean, kept
