"""NeuMF / NCF (He et al., "Neural Collaborative Filtering", WWW 2017; registry name ``neumf``) on the engine's kernels. The reference has
no such model; this one is not a port. The definitions below are the paper as remembered, not a transcription of it.

A GMF branch over tables ``pg`` [n_users, Dg], ``qg`` [n_items, Dg] and an MLP branch over tables ``pm`` [n_users, Dm], ``qm``
[n_items, Dm] with layer widths (H1, ..., HL), 0 <= L <= ``ops.NEUMF_MAX_LAYERS``, each at most ``ops.NEUMF_MAX_H``. The first layer is
stored split by side, ``W1 [pm_u ; qm_i] + b1 = (W1u pm_u + b1) + (W1i qm_i)``:

    a_u = W1u pm_u + b1          b_i = W1i qm_i
    z1  = relu(a_u + b_i)        z_l = relu(W_l z_{l-1} + b_l),  l = 2..L
    y(u, i) = <w_g, pg_u * qg_i> + <w_h, z_L> + c          (the logit: losses take logits, as everywhere here)

L = 0 with Dg > 0 is plain GMF; Dg = 0 with L >= 1 is the paper's MLP model; both empty is a ``ValueError``.

Training is the composition on the autograd tape: ``ops.LookupFn`` for the four tables, ``ops.LinearActFn`` for ``a``, ``b`` and the tail
(the GEMM family), torch elementwise operations for the add / ReLU and the last dot product, ``ops.ScoreDotFn`` for the GMF term; it returns
[B, 1 + N] logits for whichever ``rec_loss`` is configured (``bce`` is the paper's). Evaluation is full-catalogue and never forms the
[users, items, H1] activation: ``get_user_representations`` gives ``[a_u | pg_u * w_g]`` and ``get_item_representations`` ``[b_i | qg_i]``,
both plain [n, H1 + Dg] matrices, so item sharding and user chunking work unchanged; ``combine_user_item_representations`` lays the GMF
term down with the fp32 GEMM (``ops.score``) and adds the MLP term of every pair with ``ops.neumf_score_all`` (``sbr_neumf_score_all``:
fixed-order fp32 fmaf chains, no atomics, valid in deterministic mode; a pair's bits do not depend on chunking or sharding). (Training in
deterministic mode needs every width H1 .. HL in multiples of 4: ``sbr_colsum``, the gradient of ``mlp_in_bias`` and of the tail biases,
has its fixed-order form only there; the training ``forward`` says so with a ``ValueError`` before anything is launched.) A 3-D item
side (evaluation-mode ``forward`` on [B, 1 + N] batches) takes the pair-list form of the same kernel, ``ops.neumf_score_pairs``. The
packed tail weights are built once per evaluation (``get_item_representations`` builds them, ``train()`` / ``eval()`` drop them), not once
per user chunk; a ``combine`` in training mode rebuilds them on every call. The score is not a dot product of the two representations (``dot_product_score`` is False), so the fused scorers are not
offered it; with L = 0 it is one, and ``fused_score_transform`` lets GMF at Dg 64 / 128 reach them (``out_bias`` is added to the lists'
values; it does not change a ranking).

Deliberate differences from the paper: there is no pre-training schedule of our own (``load_pretrained`` is the paper's initialisation
from a trained GMF and a trained MLP; training them is the caller's); the L2 term is the optimizer's weight decay, as for every other
model here; negatives are the loader's.
"""
from __future__ import annotations

import torch
from torch import nn

from . import ops
from .sbnet import SGDBasedRecommenderAlgorithm, general_weight_init


class NeuMF(SGDBasedRecommenderAlgorithm):
    """``gmf_dim`` = Dg >= 0, ``mlp_dim`` = Dm >= 0 (ignored, and no MLP tables are made, when ``mlp_layers`` is empty), ``mlp_layers`` =
    (H1, ..., HL). state_dict keys: gmf_user.weight, gmf_item.weight, mlp_user.weight, mlp_item.weight, mlp_in_user.weight [H1, Dm],
    mlp_in_item.weight [H1, Dm], mlp_in_bias [H1], mlp_tail.{l}.weight / .bias (l = 0 .. L - 2), out_gmf [Dg], out_mlp [HL], out_bias [1];
    the GMF keys only with Dg > 0, the MLP keys only with L >= 1."""

    def __init__(self, n_users: int, n_items: int, gmf_dim: int = 8, mlp_dim: int = 32, mlp_layers=(32, 16, 8)):
        super().__init__()
        mlp_layers = tuple(int(h) for h in mlp_layers)
        gmf_dim, mlp_dim = int(gmf_dim), int(mlp_dim)
        if gmf_dim < 0:
            raise ValueError(f'NeuMF: gmf_dim={gmf_dim} is negative')
        if mlp_dim < 0:
            raise ValueError(f'NeuMF: mlp_dim={mlp_dim} is negative')
        if len(mlp_layers) > ops.NEUMF_MAX_LAYERS:
            raise ValueError(f'NeuMF: {len(mlp_layers)} MLP layers, more than {ops.NEUMF_MAX_LAYERS}')
        if any(not 1 <= h <= ops.NEUMF_MAX_H for h in mlp_layers):
            raise ValueError(f'NeuMF: mlp_layers={mlp_layers} outside [1, {ops.NEUMF_MAX_H}]')
        if not mlp_layers and gmf_dim == 0:
            raise ValueError('NeuMF: gmf_dim=0 and no MLP layers: the model would be empty')
        if mlp_layers and mlp_dim == 0:
            raise ValueError('NeuMF: mlp_dim=0 leaves the MLP without an input')
        self.n_users, self.n_items = n_users, n_items
        self.gmf_dim, self.mlp_dim, self.mlp_layers = gmf_dim, mlp_dim if mlp_layers else 0, mlp_layers
        if gmf_dim:
            self.gmf_user = nn.Embedding(n_users, gmf_dim)
            self.gmf_item = nn.Embedding(n_items, gmf_dim)
        if mlp_layers:
            self.mlp_user = nn.Embedding(n_users, mlp_dim)
            self.mlp_item = nn.Embedding(n_items, mlp_dim)
            self.mlp_in_user = nn.Linear(mlp_dim, mlp_layers[0], bias=False)
            self.mlp_in_item = nn.Linear(mlp_dim, mlp_layers[0], bias=False)
            self.mlp_tail = nn.ModuleList(nn.Linear(mlp_layers[l - 1], mlp_layers[l]) for l in range(1, len(mlp_layers)))
        self.apply(general_weight_init)
        for m in self.modules():
            if isinstance(m, nn.Embedding):
                nn.init.normal_(m.weight, std=0.01)
        if mlp_layers:
            # the first layer is one Linear over [pm ; qm]: initialised as such, stored by side so that no op sees a strided weight view
            w1 = torch.empty(mlp_layers[0], 2 * mlp_dim)
            nn.init.kaiming_uniform_(w1, nonlinearity='relu')
            with torch.no_grad():
                self.mlp_in_user.weight.copy_(w1[:, :mlp_dim])
                self.mlp_in_item.weight.copy_(w1[:, mlp_dim:])
            self.mlp_in_bias = nn.Parameter(torch.zeros(mlp_layers[0]))
        # the prediction layer is one Linear over [pg * qg ; z_L], stored by branch
        last = mlp_layers[-1] if mlp_layers else 0
        wo = torch.empty(1, gmf_dim + last)
        nn.init.kaiming_uniform_(wo, nonlinearity='relu')
        if gmf_dim:
            self.out_gmf = nn.Parameter(wo[0, :gmf_dim].clone())
        if mlp_layers:
            self.out_mlp = nn.Parameter(wo[0, gmf_dim:].clone())
        self.out_bias = nn.Parameter(torch.zeros(1))
        self._tail = None                                         # the packed tail weights of the current evaluation
        self.name = 'NeuMF'

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        keys = ('gmf_dim', 'mlp_dim', 'mlp_layers')
        return NeuMF(dataset.n_users, dataset.n_items, **{k: conf[k] for k in keys if k in conf})

    @property
    def dot_product_score(self) -> bool:
        """True when the score is the dot product of the two representations (plus ``out_bias``): plain GMF, L = 0."""
        return not self.mlp_layers

    def fused_score_transform(self):
        """``(items_fn, users_fn, finish_fn)`` for the fused full-catalogue scorers, for plain GMF (L = 0) only: the dot product of the
        representations is the GMF term itself; ``out_bias`` is added to the lists' values afterwards and changes no ranking. With MLP
        layers ``dot_product_score`` is False and the evaluation never asks; a direct call raises."""
        if self.mlp_layers:
            raise RuntimeError('NeuMF with MLP layers has no fused_score_transform: its score is not a dot product')
        bias = self.out_bias.detach()
        return None, None, lambda val, idx: (val + bias, idx)

    def train(self, mode: bool = True):
        self._tail = None
        return super().train(mode)

    def _need_cuda_idx(self, *idxs):
        if any(not t.is_cuda for t in idxs):
            raise RuntimeError('NeuMF (HIP engine) needs CUDA(HIP) index tensors')

    def packed_tail(self, rebuild: bool = False):
        """``ops.neumf_pack_tail`` of the current tail layers, kept until the next ``train()`` / ``eval()`` or ``rebuild``. In training mode
        ``combine_user_item_representations`` rebuilds it on every call: the optimizer moves the weights between two of them."""
        if self._tail is None or rebuild:
            self._tail = ops.neumf_pack_tail([m.weight for m in self.mlp_tail], [m.bias for m in self.mlp_tail], self.out_mlp, self.out_bias)
        return self._tail

    # ---- the two sides -------------------------------------------------------------------------------------------------------------------
    def _side(self, idxs, mlp_table, mlp_in, bias, gmf_table, gmf_scale):
        """[..., H1 + Dg] of the rows ``idxs``: the side's half of the first layer, then its GMF row (times ``gmf_scale``)"""
        parts = []
        flat = idxs.reshape(-1)
        if self.mlp_layers:
            parts.append(ops.LinearActFn.apply(ops.LookupFn.apply(mlp_table.weight, flat), mlp_in.weight, bias, 0))
        if self.gmf_dim:
            g = ops.LookupFn.apply(gmf_table.weight, flat)
            parts.append(g * gmf_scale if gmf_scale is not None else g)
        out = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
        return out.reshape(*idxs.shape, out.shape[1])

    def get_user_representations(self, u_idxs):
        self._need_cuda_idx(u_idxs)
        return self._side(u_idxs, getattr(self, 'mlp_user', None), getattr(self, 'mlp_in_user', None), getattr(self, 'mlp_in_bias', None),
                          getattr(self, 'gmf_user', None), getattr(self, 'out_gmf', None))

    def get_item_representations(self, i_idxs):
        self._need_cuda_idx(i_idxs)
        if self.mlp_layers and not self.training:
            self.packed_tail(rebuild=True)                        # once per evaluation: every chunk's combine reuses it
        return self._side(i_idxs, getattr(self, 'mlp_item', None), getattr(self, 'mlp_in_item', None), None,
                          getattr(self, 'gmf_item', None), None)

    def combine_user_item_representations(self, u_repr, i_repr):
        """No autograd through the MLP term: evaluation only (training scores through ``forward``)."""
        if i_repr.ndim == 3 and i_repr.shape[0] == 1:             # [1, I, .]: broadcast over users, as in SGDMatrixFactorization
            i_repr = i_repr[0]
        h1 = self.mlp_layers[0] if self.mlp_layers else 0
        u_repr, i_repr = u_repr.detach(), i_repr.detach()
        out = None
        if self.gmf_dim:
            out = ops.score(u_repr[:, h1:], i_repr[..., h1:]).detach()
        if not self.mlp_layers:
            B, N = out.shape
            return ops.BiasScoreFn.apply(out, None, None, self.out_bias.detach(), None, None, B, N)
        tail = self.packed_tail(rebuild=self.training)
        if i_repr.ndim == 2:
            return ops.neumf_score_all(u_repr[:, :h1], i_repr[:, :h1], tail, self.mlp_layers, out=out, accumulate=out is not None)
        B, N = i_repr.shape[:2]
        rows = i_repr.reshape(B * N, i_repr.shape[2])
        u_slot = torch.arange(B, device=rows.device, dtype=torch.int32).repeat_interleave(N)
        i_slot = torch.arange(B * N, device=rows.device, dtype=torch.int32)
        flat = out.contiguous().reshape(-1) if out is not None else None
        return ops.neumf_score_pairs(u_repr[:, :h1], rows[:, :h1], u_slot, i_slot, tail, self.mlp_layers, out=flat,
                                     accumulate=flat is not None).reshape(B, N)

    def forward(self, u_idxs, i_idxs):
        self._need_cuda_idx(u_idxs, i_idxs)
        if not self.training:
            with torch.no_grad():
                return self.combine_user_item_representations(self.get_user_representations(u_idxs), self.get_item_representations(i_idxs))
        if i_idxs.dim() != 2 or u_idxs.dim() != 1 or i_idxs.shape[0] != u_idxs.shape[0]:
            raise ValueError(f'NeuMF: a training batch is u_idxs [B] and i_idxs [B, 1 + N], got {tuple(u_idxs.shape)} and '
                             f'{tuple(i_idxs.shape)}')
        if ops.is_deterministic() and any(h % 4 for h in self.mlp_layers):
            raise ValueError(f'NeuMF: training in deterministic mode needs every MLP width in multiples of 4, got {self.mlp_layers}: the bias '
                             f'gradients are column sums (sbr_colsum), which have their fixed-order form only there')
        B, S = i_idxs.shape
        y = None
        if self.gmf_dim:
            pg = ops.LookupFn.apply(self.gmf_user.weight, u_idxs)
            qg = ops.LookupFn.apply(self.gmf_item.weight, i_idxs)
            y = ops.ScoreDotFn.apply(pg * self.out_gmf, qg)
        if self.mlp_layers:
            a = ops.LinearActFn.apply(ops.LookupFn.apply(self.mlp_user.weight, u_idxs), self.mlp_in_user.weight, self.mlp_in_bias, 0)
            b = ops.LinearActFn.apply(ops.LookupFn.apply(self.mlp_item.weight, i_idxs.reshape(-1)), self.mlp_in_item.weight, None, 0)
            z = torch.relu(a[:, None, :] + b.view(B, S, -1)).reshape(B * S, -1)
            for layer in self.mlp_tail:
                z = ops.LinearActFn.apply(z, layer.weight, layer.bias, ops.ACT_CODES['relu'])
            m = (z * self.out_mlp).sum(dim=1).view(B, S)
            y = m if y is None else y + m
        return y + self.out_bias

    def get_and_reset_other_loss(self):
        return {'reg_loss': torch.zeros((), device=self.device)}

    @torch.no_grad()
    def load_pretrained(self, gmf_model: 'NeuMF', mlp_model: 'NeuMF', alpha: float = 0.5):
        """The paper's initialisation from a trained GMF (``gmf_model``: L = 0) and a trained MLP (``mlp_model``: Dg = 0): tables and layers
        are copied, ``out_gmf = alpha w_gmf``, ``out_mlp = (1 - alpha) w_mlp``, ``out_bias = alpha c_gmf + (1 - alpha) c_mlp``."""
        if not 0 <= alpha <= 1:
            raise ValueError(f'NeuMF.load_pretrained: alpha={alpha} outside [0, 1]')
        if not self.gmf_dim or not self.mlp_layers:
            raise ValueError('NeuMF.load_pretrained: needs a model with both branches')
        if gmf_model.mlp_layers or gmf_model.gmf_dim != self.gmf_dim or (gmf_model.n_users, gmf_model.n_items) != (self.n_users, self.n_items):
            raise ValueError(f'NeuMF.load_pretrained: the GMF model (gmf_dim={gmf_model.gmf_dim}, mlp_layers={gmf_model.mlp_layers}, '
                             f'{gmf_model.n_users} x {gmf_model.n_items}) does not match gmf_dim={self.gmf_dim}, no MLP layers, '
                             f'{self.n_users} x {self.n_items}')
        if (mlp_model.gmf_dim or mlp_model.mlp_layers != self.mlp_layers or mlp_model.mlp_dim != self.mlp_dim
                or (mlp_model.n_users, mlp_model.n_items) != (self.n_users, self.n_items)):
            raise ValueError(f'NeuMF.load_pretrained: the MLP model (gmf_dim={mlp_model.gmf_dim}, mlp_dim={mlp_model.mlp_dim}, '
                             f'mlp_layers={mlp_model.mlp_layers}, {mlp_model.n_users} x {mlp_model.n_items}) does not match gmf_dim=0, '
                             f'mlp_dim={self.mlp_dim}, mlp_layers={self.mlp_layers}, {self.n_users} x {self.n_items}')
        mine = dict(self.named_parameters())
        for src in (gmf_model, mlp_model):
            for name, p in src.named_parameters():
                if not name.startswith('out_'):
                    mine[name].copy_(p)
        self.out_gmf.copy_(alpha * gmf_model.out_gmf)
        self.out_mlp.copy_((1. - alpha) * mlp_model.out_mlp)
        self.out_bias.copy_(alpha * gmf_model.out_bias + (1. - alpha) * mlp_model.out_bias)
        self._tail = None
        return self
