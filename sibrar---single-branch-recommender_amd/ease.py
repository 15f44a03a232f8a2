"""EASE — Embarrassingly Shallow Autoencoders (Steck 2019; algorithms/linear_algs.py:130-175) behind the reference's
``SparseMatrixBasedRecommenderAlgorithm`` surface.

``fit(matrix)`` keeps the interaction matrix resident as CSR, counts the Gram matrix ``G = X^T X + int(lam) I`` into one dense float32
[n_items, n_items] buffer (``ops.gram_dense``: integer LDS atomics, exact), inverts it in place (``ops.spd_inverse_``: the blocked symmetric
sweep of csrc/ease.hip, its rank-64 update on the fp32 matrix pipe) and turns it in place into the weights ``B = P / (-diag(P))`` with a zero
diagonal (``ops.ease_weights_``). That buffer is the model, ``self.B``; no second one of its size is allocated. The reference's ``pred_mtx``
(users x items, float64) is never built: score rows are made per user chunk by ``ops.csr_rows_times_dense`` — ``matrix[u] @ B``
(linear_algs.py:160).

Full-catalogue evaluation goes through the hooks ``evaluate_recommender_algorithm`` already calls, exactly as for the KNN models: the item
side is a 1-tuple (the item ids), which takes the ``fp32`` route.

Deliberate differences from the reference: the Gram matrix is inverted in fp32 by an unpivoted blocked sweep (the reference: float64
LAPACK), which needs a positive definite matrix, so ``int(lam) < 1`` is refused (the reference accepts it and inverts a Gram matrix that may be
singular); the interaction data must be 0/1; ``model.npz`` holds ``B``, not ``pred_mtx``, so a loaded model needs the interaction matrix again
(``attach``).
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


class EASE(SparseMatrixBasedRecommenderAlgorithm):
    """algorithms/linear_algs.py:130-175. ``lam``: the L2 regularisation; the diagonal gets ``int(lam)`` (:153). ``kwargs``: ``device``."""

    def __init__(self, lam, **kwargs):
        super().__init__()
        if int(lam) < 1:
            raise ValueError(f'lam={lam!r}: the diagonal gets int(lam) = {int(lam)} (algorithms/linear_algs.py:153), and below 1 the Gram matrix '
                             f'may be singular; the fp32 sweep needs a positive definite matrix (a deliberate difference from the reference)')
        self.lam = lam
        self.device = torch.device(kwargs.get('device') or 'cuda')
        self.B = None                          # the model: float32 [n_items, n_items]
        self.n_users = self.n_items = None
        self._matrix = None                    # DeviceCSR of the user x item matrix
        self.name = 'EASE'
        logging.info(f'Built {self.name} module \n- lam: {self.lam} ')

    def to(self, device):
        self.device = torch.device(device)
        if self._matrix is not None:
            self._matrix = self._matrix.to(self.device)
        if self.B is not None:
            self.B = self.B.to(self.device)
        return self

    # ---- fitting ----------------------------------------------------------------------------------------------------------------
    def attach(self, matrix: sp.spmatrix):
        """Make the user x item matrix resident without fitting: what a model loaded from ``model.npz`` needs before it can score."""
        try:
            m = _binary_csr(matrix)
        except ValueError:
            raise ValueError('EASE: the Gram matrix is counted with integer atomics, and its entries are integer counts for 0/1 interaction '
                             'data only: the matrix has entries other than 1 (after sum_duplicates / eliminate_zeros)') from None
        self.n_users, self.n_items = m.shape
        self._matrix = DeviceCSR(m).to(self.device)
        return self

    def fit(self, matrix: sp.spmatrix, **kwargs):
        """:param matrix: user x item sparse matrix"""
        self.attach(matrix)
        self.B = None
        G = ops.gram_dense(self._matrix, float(int(self.lam)))            # linear_algs.py:150-153
        self.B = ops.ease_weights_(ops.spd_inverse_(G))                  # :155-158, both in place
        return self

    def _need_fit(self):
        if self.B is None:
            raise RuntimeError(f'{self.name}: no weights, run fit(matrix) or load_model_from_path(path)')

    def _rows(self, u: torch.Tensor) -> torch.Tensor:
        self._need_fit()
        if self._matrix is None:
            raise RuntimeError(f'{self.name}: the weights were loaded from model.npz, which does not hold the interactions: call '
                               f'attach(matrix) with the user x item matrix first')
        if tuple(self.B.shape) != (self.n_items, self.n_items):
            raise ValueError(f'{self.name}: weights of shape {tuple(self.B.shape)} do not fit the {self.n_items} items of the matrix')
        if self.B.device != self.device:
            self.B = self.B.to(self.device)
        return ops.csr_rows_times_dense(self._matrix, u, self.B)

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
        np.savez(os.path.join(path, 'model.npz'), B=self.B.cpu().numpy(), lam=np.array(self.lam), name=np.array(self.name))
        print('Model Saved')

    def load_model_from_path(self, path: str, matrix: sp.spmatrix = None):
        with np.load(os.path.join(path, 'model.npz'), allow_pickle=False) as f:
            if 'pred_mtx' in f.files or 'B' not in f.files:
                raise ValueError(f'{os.path.join(path, "model.npz")} is not a model of this package (it holds {f.files}): the reference '
                                 f'stores its pickled prediction matrix `pred_mtx`, this package the item-item weights; fit the model again')
            name, B = str(f['name']), f['B']
        if name != self.name:
            raise ValueError(f'model.npz holds a {name}, this model is a {self.name}')
        if B.ndim != 2 or B.shape[0] != B.shape[1]:
            raise ValueError(f'model.npz: weights of shape {B.shape} are not square')
        self.B = torch.from_numpy(B.astype(np.float32))
        if matrix is not None:
            self.attach(matrix)
        print('Model Loaded')

    @staticmethod
    def build_from_conf(conf: dict, dataset=None):
        return EASE(conf['lam'])
