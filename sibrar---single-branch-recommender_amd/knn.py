"""Neighbourhood models on the sparse user x item matrix: ``UserKNN`` / ``ItemKNN`` (algorithms/knn_algs.py) behind the reference's
``SparseMatrixBasedRecommenderAlgorithm`` surface (algorithms/base_classes.py:54-84), with the similarity functions of
utilities/similarities.py named by ``SimilarityFunctionEnum``.

``fit(matrix)`` keeps the interaction matrix resident as CSR and runs ``ops.knn_topk`` (csrc/knn.hip: co-occurrence counts by integer LDS
atomics, similarity and top-k selection of a row inside one workgroup); what it keeps is the neighbour lists ``(nbr_idx, nbr_val, nbr_len)``
and their CSR form S. The reference's ``pred_mtx`` (users x items, densified at the first ``predict``) is never built: score rows are made
per user chunk by ``ops.csr_rows_times_csr`` — ``S[u] @ matrix`` (UserKNN, knn_algs.py:96) or ``matrix[u] @ S^T`` (ItemKNN, knn_algs.py:116).

Full-catalogue evaluation goes through the hooks ``evaluate_recommender_algorithm`` already calls: the item side is a 1-tuple (the item ids),
which takes the ``fp32`` route — score rows, exclusion mask, exact top-k — whatever ``scorer`` asks for.

``ItemFeatureKNN`` compares dense item feature rows instead (``ops.dense_knn_topk``, csrc/dense_knn.hip: the n x n x d product on the fp32
matrix pipe with the cosine value and the top-k selection on chip) and predicts as ItemKNN does; see its docstring.

Deliberate differences from the reference: the similarities are computed in fp32 (the reference: float64) in the operation order stated in
include/sibrar_hip.h; among equal similarities at the k-th place the lower index is kept (the reference: whichever an unstable argsort
leaves); ``model.npz`` holds the lists, not ``pred_mtx``, so a loaded model needs the interaction matrix again (``attach``).
"""
from __future__ import annotations

import logging
from abc import ABC
from enum import Enum

import numpy as np
import scipy.sparse as sp
import torch

from . import ops
from .features import DeviceCSR
from .matrix_models import ResidentMatrixAlgorithm, SparseMatrixBasedRecommenderAlgorithm, _binary_csr      # noqa: F401


class SimilarityFunctionEnum(Enum):
    """utilities/similarities.py:133-139, by name (the reference's values are its SciPy functions)."""
    jaccard = 'jaccard'
    cosine = 'cosine'
    dense_cosine = 'dense_cosine'
    asymmetric_cosine = 'asymmetric_cosine'
    tversky = 'tversky'
    sorensen_dice = 'sorensen_dice'


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


class KNNAlgorithm(ResidentMatrixAlgorithm, ABC):
    """algorithms/knn_algs.py:13-76. ``kwargs``: ``alpha`` (asymmetric_cosine, tversky), ``beta`` (tversky), ``device``."""
    ENTITY = None            # 'user' | 'item': whose rows are compared
    KEY, WHAT, STORES = 'nbr_idx', 'neighbour lists', 'the neighbour lists'
    BINARY_ONLY = 'KNN similarities are stated for 0/1 interaction data only (utilities/similarities.py:11-15)'
    DENSE = False            # the rows compared are dense feature rows (dense_cosine) rather than rows of the 0/1 matrix
    SIM_REFUSAL = ('dense_cosine is the similarity of ItemFeatureKNN (ifknn), which compares dense feature rows; uknn / iknn compare rows '
                   'of the 0/1 matrix and take jaccard, cosine, asymmetric_cosine, tversky or sorensen_dice')

    def __init__(self, sim_func_enum: SimilarityFunctionEnum = SimilarityFunctionEnum.cosine, k: int = 100, shrinkage: float = .0, **kwargs):
        super().__init__(kwargs.get('device'))
        if isinstance(sim_func_enum, str):
            sim_func_enum = SimilarityFunctionEnum[sim_func_enum]
        if (sim_func_enum == SimilarityFunctionEnum.dense_cosine) != self.DENSE:
            raise ValueError(self.SIM_REFUSAL)
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
        self.nbr_idx = self.nbr_val = self.nbr_len = None      # the model: int32 [n, k], float32 [n, k], int32 [n]
        self._operands = None                                   # (X, Y) of ops.csr_rows_times_csr
        self.name = 'KNNAlgorithm'
        logging.info(f'Built {self.name} module \n- sim_func: {self.sim_func_enum.name} \n- k: {self.k} \n- shrinkage: {self.shrinkage} \n')

    def to(self, device):
        self._operands = None
        return super().to(device)

    def _resident(self, m):
        """the compared rows: users x items, or items x users"""
        self._operands = None
        return DeviceCSR(m if self.ENTITY == 'user' else sp.csr_matrix(m.T))

    def fit(self, matrix: sp.spmatrix, **kwargs):
        """:param matrix: user x item sparse matrix"""
        self.attach(matrix)
        self.nbr_idx, self.nbr_val, self.nbr_len = ops.knn_topk(self._matrix, self.sim_func_enum.name, self.k, self.shrinkage, self.alpha,
                                                                self.beta)
        return self

    def similarity_csr(self):
        """S [n, n] as ``(indptr, indices, data, shape)`` on the model's device, columns ascending."""
        self._need_fit()
        return _lists_to_csr(self.nbr_idx.to(self.device), self.nbr_val.to(self.device), self.nbr_len.to(self.device), False)

    def _ops(self):
        """(X, Y) of ``ops.csr_rows_times_csr``, of a fitted model with its matrix resident"""
        if self._operands is None:
            n = self.n_users if self.ENTITY == 'user' else self.n_items
            if tuple(self.nbr_idx.shape) != (n, self.k) or int(self.nbr_len.numel()) != n:
                raise ValueError(f'{self.name}: lists of shape {tuple(self.nbr_idx.shape)} do not fit the {n} {self.ENTITY}s of the matrix')
            lists = (self.nbr_idx.to(self.device), self.nbr_val.to(self.device), self.nbr_len.to(self.device))
            if self.ENTITY == 'user':           # sim_mtx @ matrix
                self._operands = (_lists_to_csr(*lists, False), self._matrix)
            else:                               # matrix @ sim_mtx.T; the resident matrix is items x users: its transpose is the matrix
                t_indptr, t_indices, _ = self._matrix.transposed()
                self._operands = ((t_indptr, t_indices, None, (self.n_users, self.n_items)), _lists_to_csr(*lists, True))
        return self._operands

    def _score_rows(self, u):
        x, y = self._ops()
        return ops.csr_rows_times_csr(x, u, y)

    def _npz_fields(self):
        return dict(nbr_idx=self.nbr_idx.cpu().numpy(), nbr_val=self.nbr_val.cpu().numpy(), nbr_len=self.nbr_len.cpu().numpy(),
                    k=np.array(self.k), sim_func=np.array(self.sim_func_enum.name))

    def _read_npz(self, f):
        k, sim = int(f['k']), str(f['sim_func'])
        if (k, sim) != (self.k, self.sim_func_enum.name):
            raise ValueError(f'model.npz holds a {self.name} (k={k}, {sim}), this model is a {self.name} (k={self.k}, {self.sim_func_enum.name})')
        idx, val, length = f['nbr_idx'], f['nbr_val'], f['nbr_len']
        if idx.shape != val.shape or idx.ndim != 2 or idx.shape[1] != k or length.shape != (idx.shape[0],):
            raise ValueError(f'model.npz: inconsistent list shapes {idx.shape}, {val.shape}, {length.shape}')
        self.nbr_idx, self.nbr_val = torch.from_numpy(idx.astype(np.int32)), torch.from_numpy(val.astype(np.float32))
        self.nbr_len = torch.from_numpy(length.astype(np.int32))
        self._operands = None

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
            return ItemFeatureKNN(sim_func, conf['k'], shrinkage)
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


def _dense_features(feature_matrix, n_items: int, device) -> torch.Tensor:
    """``feature_matrix`` (np.ndarray, torch.Tensor or scipy sparse) as a finite float32 [n_items, d] tensor on ``device``"""
    if feature_matrix is None:
        raise ValueError('ItemFeatureKNN.fit needs feature_matrix: the dense item x feature_dim matrix (algorithms/knn_algs.py:129-133)')
    if sp.issparse(feature_matrix):
        feature_matrix = feature_matrix.toarray()
    f = feature_matrix.detach() if isinstance(feature_matrix, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(feature_matrix))
    if f.dim() != 2 or f.shape[0] != n_items or f.shape[1] < 1:
        raise ValueError(f'ItemFeatureKNN.fit: feature_matrix of shape {tuple(f.shape)}, expected [{n_items} items, d >= 1]')
    f = f.to(device=device, dtype=torch.float32).contiguous()
    if not bool(torch.isfinite(f).all()):
        raise ValueError('ItemFeatureKNN.fit: feature_matrix has entries that are not finite (after the cast to float32)')
    return f


class ItemFeatureKNN(KNNAlgorithm):
    """algorithms/knn_algs.py:121-140: items similar by their dense features (``dense_cosine``, utilities/similarities.py:86-93);
    ``pred = matrix @ sim_mtx.T`` as ItemKNN. ``fit(matrix, feature_matrix)``; the features are not kept: the model is the lists.

    What the reference does and this model keeps: the candidates of an item are the items with a non-zero dot product, itself included
    with the value 0, so a list of fewer than k positive similarities goes on with that explicit 0 and then the negative ones; an
    all-zero feature row has an empty list. Deliberate differences: fp32 instead of float64 (the order of include/sibrar_hip.h); the
    lowest index wins among equal values (the reference: whichever an unstable argsort leaves); ``dense_cosine`` only, and as the
    constructor's default (the reference's default, cosine, is stated for 0/1 rows); ``shrinkage > 0`` only with features that are all
    >= 0 — the factor dot / (dot + shrinkage) has a pole at dot = -shrinkage, and the reference returns "similarities" of any size
    around it; ``model.npz`` holds the lists and needs ``attach(matrix)``; ``k <= 256``."""
    ENTITY = 'item'
    DENSE = True
    SIM_REFUSAL = ('ifknn (ItemFeatureKNN) compares dense feature rows and takes dense_cosine only; jaccard, cosine, asymmetric_cosine, '
                   'tversky and sorensen_dice are stated for rows of the 0/1 matrix (uknn / iknn)')

    def __init__(self, sim_func: SimilarityFunctionEnum = SimilarityFunctionEnum.dense_cosine, k: int = 100, shrinkage: float = .0, **kwargs):
        super().__init__(sim_func, k, shrinkage, **kwargs)
        self.name = 'ItemFeatureKNN'
        logging.info(f'Built {self.name} module \n')

    def fit(self, matrix: sp.spmatrix, feature_matrix=None, **kwargs):
        """:param matrix: user x item sparse matrix
        :param feature_matrix: item x feature_dim matrix: np.ndarray, torch.Tensor or scipy sparse (densified)"""
        self.attach(matrix)
        f = _dense_features(feature_matrix, self.n_items, self.device)
        if self.shrinkage > 0 and bool((f < 0).any()):
            raise ValueError(f'ItemFeatureKNN: shrinkage={self.shrinkage} with negative features: the factor dot / (dot + shrinkage) has a '
                             f'pole at dot = -shrinkage, so negative dot products give values of any size and sign; use shrinkage=0 or '
                             f'features that are all >= 0')
        self.nbr_idx, self.nbr_val, self.nbr_len = ops.dense_knn_topk(f, self.k, self.shrinkage)
        self._operands = None
        return self
