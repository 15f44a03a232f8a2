"""Neighbourhood models on the sparse user x item matrix: ``UserKNN`` / ``ItemKNN`` (algorithms/knn_algs.py) behind the reference's
``SparseMatrixBasedRecommenderAlgorithm`` surface (algorithms/base_classes.py:54-84), with the similarity functions of
utilities/similarities.py named by ``SimilarityFunctionEnum``.

``fit(matrix)`` keeps the interaction matrix resident as CSR and runs ``ops.knn_topk`` (csrc/knn.hip: co-occurrence counts by integer LDS
atomics, similarity and top-k selection of a row inside one workgroup); what it keeps is the neighbour lists ``(nbr_idx, nbr_val, nbr_len)``
and their CSR form S. The reference's ``pred_mtx`` (users x items, densified at the first ``predict``) is never built: score rows are made
per user chunk by ``ops.csr_rows_times_csr`` — ``S[u] @ matrix`` (UserKNN, knn_algs.py:96) or ``matrix[u] @ S^T`` (ItemKNN, knn_algs.py:116).

Full-catalogue evaluation goes through the hooks ``evaluate_recommender_algorithm`` already calls: the item side is a 1-tuple (the item ids),
which takes the ``fp32`` route — score rows, exclusion mask, exact top-k — whatever ``scorer`` asks for.

Deliberate differences from the reference: the similarities are computed in fp32 (the reference: float64) in the operation order stated in
include/sibrar_hip.h; among equal similarities at the k-th place the lower index is kept (the reference: whichever an unstable argsort
leaves); ``model.npz`` holds the lists, not ``pred_mtx``, so a loaded model needs the interaction matrix again (``attach``).
"""
from __future__ import annotations

import logging
import os
from abc import ABC, abstractmethod
from enum import Enum

import numpy as np
import scipy.sparse as sp
import torch

from . import ops
from .features import DeviceCSR


class SimilarityFunctionEnum(Enum):
    """utilities/similarities.py:133-139, by name (the reference's values are its SciPy functions)."""
    jaccard = 'jaccard'
    cosine = 'cosine'
    dense_cosine = 'dense_cosine'
    asymmetric_cosine = 'asymmetric_cosine'
    tversky = 'tversky'
    sorensen_dice = 'sorensen_dice'


class SparseMatrixBasedRecommenderAlgorithm(ABC):
    """algorithms/base_classes.py:54-84 — algorithms trained from the sparse user x item matrix by ``fit(matrix)``; no Trainer. ``eval()`` /
    ``train()`` exist so that the evaluation loop's ``alg.eval()`` works; there is no mode to switch."""

    def __init__(self):
        self.name = 'SparseMatrixBasedRecommenderAlgorithm'
        logging.info(f'Built {self.name} module')

    @abstractmethod
    def fit(self, matrix: sp.spmatrix, **kwargs):
        """:param matrix: user x item sparse matrix"""

    @abstractmethod
    def predict(self, u_idxs: torch.Tensor, i_idxs: torch.Tensor) -> torch.Tensor:
        """u_idxs [batch_size], i_idxs [batch_size, n] -> scores [batch_size, n]"""

    @abstractmethod
    def save_model_to_path(self, path: str):
        pass

    @abstractmethod
    def load_model_from_path(self, path: str):
        pass

    @staticmethod
    @abstractmethod
    def build_from_conf(conf: dict, dataset):
        pass

    def eval(self):
        return self

    def train(self, mode: bool = True):
        return self


def _binary_csr(matrix) -> sp.csr_matrix:
    m = sp.csr_matrix(matrix).copy()
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    if m.nnz and bool((m.data != 1).any()):
        raise ValueError('KNN similarities are stated for 0/1 interaction data only (utilities/similarities.py:11-15): the matrix has '
                         'entries other than 1 (after sum_duplicates / eliminate_zeros)')
    return m


def _lists_to_csr(idx: torch.Tensor, val: torch.Tensor, length: torch.Tensor, transpose: bool):
    """The neighbour lists as CSR ``(indptr, indices, data, shape)`` with ascending columns — S, or S^T built from the same entries."""
    n, k = idx.shape
    keep = torch.arange(k, device=idx.device)[None, :] < length[:, None]
    rows = torch.arange(n, device=idx.device)[:, None].expand(n, k)[keep]
    cols, data = idx[keep].long(), val[keep]
    if transpose:
        rows, cols = cols, rows
    order = torch.argsort(rows * n + cols)
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=idx.device)
    indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    return indptr, cols[order].to(torch.int32).contiguous(), data[order].contiguous(), (n, n)


class KNNAlgorithm(SparseMatrixBasedRecommenderAlgorithm, ABC):
    """algorithms/knn_algs.py:13-76. ``kwargs``: ``alpha`` (asymmetric_cosine, tversky), ``beta`` (tversky), ``device``."""
    ENTITY = None            # 'user' | 'item': whose rows are compared

    def __init__(self, sim_func_enum: SimilarityFunctionEnum = SimilarityFunctionEnum.cosine, k: int = 100, shrinkage: float = .0, **kwargs):
        super().__init__()
        if isinstance(sim_func_enum, str):
            sim_func_enum = SimilarityFunctionEnum[sim_func_enum]
        if sim_func_enum == SimilarityFunctionEnum.dense_cosine:
            raise ValueError('dense_cosine is the similarity of ItemFeatureKNN (ifknn), which this package does not provide; '
                             'uknn / iknn take jaccard, cosine, asymmetric_cosine, tversky or sorensen_dice')
        if not (isinstance(k, (int, np.integer)) and 1 <= k <= ops.KNN_MAX_K):
            raise ValueError(f'k={k!r} outside [1, {ops.KNN_MAX_K}] (the longest list the selection kernels keep)')
        if shrinkage < 0:
            raise ValueError(f'negative shrinkage {shrinkage}')
        self.sim_func_enum = sim_func_enum
        self.alpha = self.beta = None
        if sim_func_enum in (SimilarityFunctionEnum.asymmetric_cosine, SimilarityFunctionEnum.tversky):
            self.alpha = float(kwargs['alpha'])
        if sim_func_enum == SimilarityFunctionEnum.tversky:
            self.beta = float(kwargs['beta'])
        self.k = int(k)
        self.shrinkage = float(shrinkage)
        self.device = torch.device(kwargs.get('device') or 'cuda')
        self.nbr_idx = self.nbr_val = self.nbr_len = None      # the model: int32 [n, k], float32 [n, k], int32 [n]
        self.n_users = self.n_items = None
        self._entity = None                                     # DeviceCSR of the compared rows (users x items, or items x users)
        self._operands = None                                   # (X, Y) of ops.csr_rows_times_csr
        self.name = 'KNNAlgorithm'
        logging.info(f'Built {self.name} module \n- sim_func: {self.sim_func_enum.name} \n- k: {self.k} \n- shrinkage: {self.shrinkage} \n')

    def to(self, device):
        self.device = torch.device(device)
        self._operands = None
        if self._entity is not None:
            self._entity = self._entity.to(self.device)
        return self

    # ---- fitting ----------------------------------------------------------------------------------------------------------------
    def attach(self, matrix: sp.spmatrix):
        """Make the user x item matrix resident without fitting: what a model loaded from ``model.npz`` needs before it can score."""
        m = _binary_csr(matrix)
        self.n_users, self.n_items = m.shape
        self._entity = DeviceCSR(m if self.ENTITY == 'user' else sp.csr_matrix(m.T)).to(self.device)
        self._operands = None
        return self

    def fit(self, matrix: sp.spmatrix, **kwargs):
        """:param matrix: user x item sparse matrix"""
        self.attach(matrix)
        self.nbr_idx, self.nbr_val, self.nbr_len = ops.knn_topk(self._entity, self.sim_func_enum.name, self.k, self.shrinkage, self.alpha,
                                                                self.beta)
        return self

    def similarity_csr(self):
        """S [n, n] as ``(indptr, indices, data, shape)`` on the model's device, columns ascending."""
        self._need_fit()
        return _lists_to_csr(self.nbr_idx.to(self.device), self.nbr_val.to(self.device), self.nbr_len.to(self.device), False)

    def _need_fit(self):
        if self.nbr_idx is None:
            raise RuntimeError(f'{self.name}: no neighbour lists, run fit(matrix) or load_model_from_path(path)')

    def _ops(self):
        if self._operands is None:
            self._need_fit()
            if self._entity is None:
                raise RuntimeError(f'{self.name}: the lists were loaded from model.npz, which does not hold the interactions: call '
                                   f'attach(matrix) with the user x item matrix first')
            n = self.n_users if self.ENTITY == 'user' else self.n_items
            if tuple(self.nbr_idx.shape) != (n, self.k) or int(self.nbr_len.numel()) != n:
                raise ValueError(f'{self.name}: lists of shape {tuple(self.nbr_idx.shape)} do not fit the {n} {self.ENTITY}s of the matrix')
            lists = (self.nbr_idx.to(self.device), self.nbr_val.to(self.device), self.nbr_len.to(self.device))
            if self.ENTITY == 'user':           # sim_mtx @ matrix
                self._operands = (_lists_to_csr(*lists, False), self._entity)
            else:                               # matrix @ sim_mtx.T; the entity matrix is items x users: its transpose is the matrix
                t_indptr, t_indices, _ = self._entity.transposed()
                self._operands = ((t_indptr, t_indices, None, (self.n_users, self.n_items)), _lists_to_csr(*lists, True))
        return self._operands

    # ---- scoring: the hooks of evaluate_recommender_algorithm ----------------------------------------------------------------------------
    def get_user_representations(self, u_idxs: torch.Tensor):
        return torch.as_tensor(u_idxs).long().to(self.device)

    def get_item_representations(self, i_idxs: torch.Tensor):
        return (torch.as_tensor(i_idxs).long().to(self.device),)

    def combine_user_item_representations(self, u_repr, i_repr) -> torch.Tensor:
        """-> float32 [len(u_repr), len(items)]: the users' score rows, restricted to the named item columns"""
        x, y = self._ops()
        rows = ops.csr_rows_times_csr(x, u_repr, y)
        items = i_repr[0]
        if items.dim() == 1 and items.numel() == self.n_items and bool((items == torch.arange(self.n_items, device=items.device)).all()):
            return rows
        return rows[:, items] if items.dim() == 1 else torch.gather(rows, 1, items)

    @torch.no_grad()
    def predict(self, u_idxs: torch.Tensor, i_idxs: torch.Tensor) -> torch.Tensor:
        """algorithms/base_classes.py:73-84: ``pred_mtx[u_idxs[:, None], i_idxs]``"""
        u = self.get_user_representations(u_idxs)
        x, y = self._ops()
        return torch.gather(ops.csr_rows_times_csr(x, u, y), 1, torch.as_tensor(i_idxs).long().to(self.device))

    # ---- persistence -------------------------------------------------------------------------------------------------------------------
    def save_model_to_path(self, path: str):
        self._need_fit()
        np.savez(os.path.join(path, 'model.npz'), nbr_idx=self.nbr_idx.cpu().numpy(), nbr_val=self.nbr_val.cpu().numpy(),
                 nbr_len=self.nbr_len.cpu().numpy(), name=np.array(self.name), k=np.array(self.k), sim_func=np.array(self.sim_func_enum.name))
        print('Model Saved')

    def load_model_from_path(self, path: str, matrix: sp.spmatrix = None):
        with np.load(os.path.join(path, 'model.npz'), allow_pickle=False) as f:
            if 'pred_mtx' in f.files or 'nbr_idx' not in f.files:
                raise ValueError(f'{os.path.join(path, "model.npz")} is not a model of this package (it holds {f.files}): the reference '
                                 f'stores its pickled prediction matrix `pred_mtx`, this package the neighbour lists; fit the model again')
            name, k, sim = str(f['name']), int(f['k']), str(f['sim_func'])
            if (name, k, sim) != (self.name, self.k, self.sim_func_enum.name):
                raise ValueError(f'model.npz holds a {name} (k={k}, {sim}), this model is a {self.name} (k={self.k}, {self.sim_func_enum.name})')
            idx, val, length = f['nbr_idx'], f['nbr_val'], f['nbr_len']
        if idx.shape != val.shape or idx.ndim != 2 or idx.shape[1] != k or length.shape != (idx.shape[0],):
            raise ValueError(f'model.npz: inconsistent list shapes {idx.shape}, {val.shape}, {length.shape}')
        self.nbr_idx, self.nbr_val = torch.from_numpy(idx.astype(np.int32)), torch.from_numpy(val.astype(np.float32))
        self.nbr_len = torch.from_numpy(length.astype(np.int32))
        self._operands = None
        if matrix is not None:
            self.attach(matrix)
        print('Model Loaded')

    @staticmethod
    def build_from_conf(conf: dict, dataset=None):
        sim_func_params = conf['sim_func_params']
        sim_func = SimilarityFunctionEnum[sim_func_params['sim_func_name']]
        alpha, beta = sim_func_params.get('alpha'), sim_func_params.get('beta')
        shrinkage = conf['shrinkage'] if 'shrinkage' in conf else .0
        if conf['alg'] == 'uknn':
            return UserKNN(sim_func, conf['k'], shrinkage, alpha=alpha, beta=beta)
        if conf['alg'] == 'iknn':
            return ItemKNN(sim_func, conf['k'], shrinkage, alpha=alpha, beta=beta)
        if conf['alg'] == 'ifknn':
            raise ValueError('ifknn (ItemFeatureKNN) is not provided by this package')
        raise ValueError(f"{conf['alg']} is an invalid model for KNNAlgorithm")


class UserKNN(KNNAlgorithm):
    """algorithms/knn_algs.py:80-97: similar users; ``pred = sim_mtx @ matrix``."""
    ENTITY = 'user'

    def __init__(self, sim_func: SimilarityFunctionEnum = SimilarityFunctionEnum.cosine, k: int = 100, shrinkage: float = .0, **kwargs):
        super().__init__(sim_func, k, shrinkage, **kwargs)
        self.name = 'UserKNN'
        logging.info(f'Built {self.name} module \n')


class ItemKNN(KNNAlgorithm):
    """algorithms/knn_algs.py:100-118: similar items; ``pred = matrix @ sim_mtx.T``."""
    ENTITY = 'item'

    def __init__(self, sim_func: SimilarityFunctionEnum = SimilarityFunctionEnum.cosine, k: int = 100, shrinkage: float = .0, **kwargs):
        super().__init__(sim_func, k, shrinkage, **kwargs)
        self.name = 'ItemKNN'
        logging.info(f'Built {self.name} module \n')
