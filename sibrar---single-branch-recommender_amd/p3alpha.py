"""P3alpha — the three-step random walk of Cooper et al. (WWW 2014; algorithms/graph_algs.py:9-88) behind the reference's
``SparseMatrixBasedRecommenderAlgorithm`` surface.

The reference builds the (U + I) x (U + I) transition matrix ``P = D^-1 A`` of the bipartite user-item graph, cubes it and keeps the
users x items block raised elementwise to ``alpha``. Written out, that block is ``(D_u^-1 X)(D_i^-1 X^T)(D_u^-1 X)`` with ``d_u`` and ``d_i``
the row and column sums of X. ``fit(matrix)`` keeps the interaction matrix resident as CSR and computes the last two factors as one dense
float32 [n_items, n_items] buffer ``W = D_i^-1 X^T D_u^-1 X`` (``ops.p3_walk_dense``: fixed-order fp32 sums, no atomics). That buffer is
the model, ``self.W``. The reference's ``pred_mtx`` (users x items) is never built: score rows are made per user chunk by
``ops.p3_score_rows`` — ``((D_u^-1 X)[u] @ W) ** alpha``; a zero stays zero, as in the reference's sparse ``.power``.

Full-catalogue evaluation goes through the hooks ``evaluate_recommender_algorithm`` already calls, exactly as for EASE and the KNN models:
the item side is a 1-tuple (the item ids), which takes the ``fp32`` route.

Deliberate differences from the reference: the interaction data must be 0/1 (the reference takes weights: its degrees are weighted sums);
``alpha == 0`` is refused at construction (the reference accepts it there and fails in ``fit``: scipy refuses a zero power); everything is
fp32 (the reference: float64); ``model.npz`` holds ``W``, not the pickled sparse ``pred_mtx``, so a loaded model needs the interaction
matrix again (``attach``). Users and items without interactions give zero rows, where the reference's ``1 / 0`` only raises a numpy
warning and gives the same zeros.
"""
from __future__ import annotations

import logging
import os

import numpy as np
import scipy.sparse as sp
import torch

from . import ops
from .features import DeviceCSR
from .knn import SparseMatrixBasedRecommenderAlgorithm, _binary_csr


class P3alpha(SparseMatrixBasedRecommenderAlgorithm):
    """algorithms/graph_algs.py:9-88. ``alpha``: the elementwise power of the walk probabilities (:68). ``kwargs``: ``device``."""

    def __init__(self, alpha: float = 1.9, **kwargs):
        super().__init__()
        if alpha < 0:
            raise ValueError(f'Alpha ({alpha}) has to be greater or equal than 0')              # graph_algs.py:18 asserts
        if alpha == 0:
            raise ValueError('alpha=0: the reference accepts it at construction and its fit fails (scipy refuses a zero power, '
                             'algorithms/graph_algs.py:68); refused here at once (a deliberate difference from the reference)')
        self.alpha = alpha
        self.device = torch.device(kwargs.get('device') or 'cuda')
        self.W = None                          # the model: float32 [n_items, n_items]
        self.n_users = self.n_items = None
        self._matrix = None                    # DeviceCSR of the user x item matrix
        self.name = 'P3alpha'
        logging.info(f'Built {self.name} module \n- alpha: {self.alpha}')

    def to(self, device):
        self.device = torch.device(device)
        if self._matrix is not None:
            self._matrix = self._matrix.to(self.device)
        if self.W is not None:
            self.W = self.W.to(self.device)
        return self

    # ---- fitting ----------------------------------------------------------------------------------------------------------------
    def attach(self, matrix: sp.spmatrix):
        """Make the user x item matrix resident without fitting: what a model loaded from ``model.npz`` needs before it can score."""
        try:
            m = _binary_csr(matrix)
        except ValueError:
            raise ValueError('P3alpha: the walk is computed from entry counts, which are the degrees for 0/1 interaction data only: the '
                             'matrix has entries other than 1 (after sum_duplicates / eliminate_zeros)') from None
        self.n_users, self.n_items = m.shape
        self._matrix = DeviceCSR(m).to(self.device)
        return self

    def fit(self, matrix: sp.spmatrix, **kwargs):
        """:param matrix: user x item sparse matrix"""
        self.attach(matrix)
        self.W = None
        self.W = ops.p3_walk_dense(self._matrix)                          # graph_algs.py:35-59
        return self

    def _need_fit(self):
        if self.W is None:
            raise RuntimeError(f'{self.name}: no weights, run fit(matrix) or load_model_from_path(path)')

    def _rows(self, u: torch.Tensor) -> torch.Tensor:
        self._need_fit()
        if self._matrix is None:
            raise RuntimeError(f'{self.name}: the weights were loaded from model.npz, which does not hold the interactions: call '
                               f'attach(matrix) with the user x item matrix first')
        if tuple(self.W.shape) != (self.n_items, self.n_items):
            raise ValueError(f'{self.name}: weights of shape {tuple(self.W.shape)} do not fit the {self.n_items} items of the matrix')
        if self.W.device != self.device:
            self.W = self.W.to(self.device)
        return ops.p3_score_rows(self._matrix, u, self.W, self.alpha)     # graph_algs.py:59-68

    # ---- scoring: the hooks of evaluate_recommender_algorithm ----------------------------------------------------------------------------
    def get_user_representations(self, u_idxs: torch.Tensor):
        return torch.as_tensor(u_idxs).long().to(self.device)

    def get_item_representations(self, i_idxs: torch.Tensor):
        return (torch.as_tensor(i_idxs).long().to(self.device),)

    @torch.no_grad()
    def combine_user_item_representations(self, u_repr, i_repr) -> torch.Tensor:
        """-> float32 [len(u_repr), len(items)]: the users' score rows, restricted to the named item columns"""
        rows = self._rows(u_repr)
        items = i_repr[0]
        if items.dim() == 1 and items.numel() == self.n_items and bool((items == torch.arange(self.n_items, device=items.device)).all()):
            return rows
        return rows[:, items] if items.dim() == 1 else torch.gather(rows, 1, items)

    @torch.no_grad()
    def predict(self, u_idxs: torch.Tensor, i_idxs: torch.Tensor) -> torch.Tensor:
        """algorithms/base_classes.py:73-84: ``pred_mtx[u_idxs[:, None], i_idxs]``"""
        return torch.gather(self._rows(self.get_user_representations(u_idxs)), 1, torch.as_tensor(i_idxs).long().to(self.device))

    # ---- persistence -------------------------------------------------------------------------------------------------------------------
    def save_model_to_path(self, path: str):
        self._need_fit()
        np.savez(os.path.join(path, 'model.npz'), W=self.W.cpu().numpy(), alpha=np.array(self.alpha), name=np.array(self.name))
        print('Model Saved')

    def load_model_from_path(self, path: str, matrix: sp.spmatrix = None):
        with np.load(os.path.join(path, 'model.npz'), allow_pickle=False) as f:
            if 'pred_mtx' in f.files or 'W' not in f.files:
                raise ValueError(f'{os.path.join(path, "model.npz")} is not a model of this package (it holds {f.files}): the reference '
                                 f'stores its pickled sparse prediction matrix `pred_mtx`, this package the item-item matrix of the walk; '
                                 f'fit the model again')
            name, W = str(f['name']), f['W']
        if name != self.name:
            raise ValueError(f'model.npz holds a {name}, this model is a {self.name}')
        if W.ndim != 2 or W.shape[0] != W.shape[1]:
            raise ValueError(f'model.npz: weights of shape {W.shape} are not square')
        self.W = torch.from_numpy(W.astype(np.float32))
        if matrix is not None:
            self.attach(matrix)
        print('Model Loaded')

    @staticmethod
    def build_from_conf(conf: dict, dataset=None):
        return P3alpha(alpha=conf['alpha'])
