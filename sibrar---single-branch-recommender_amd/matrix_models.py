"""The models trained from the sparse user x item matrix by ``fit(matrix)``: the reference's ``SparseMatrixBasedRecommenderAlgorithm``
surface (algorithms/base_classes.py:54-84) and what every such model of this package shares.

``ResidentMatrixAlgorithm`` keeps the 0/1 interaction matrix resident as CSR and never builds the reference's ``pred_mtx`` (users x items):
a model supplies the score rows of a user chunk, and the hooks ``evaluate_recommender_algorithm`` calls, ``predict`` and the ``model.npz``
skeleton are written here once. ``model.npz`` holds the model, not ``pred_mtx``, so a loaded model needs the interaction matrix again
(``attach``). ``DenseItemModel`` adds what the models share whose model is one dense float32 [n_items, n_items] tensor (EASE, P3alpha).

A model writes: its constructor, ``fit``, ``_score_rows``, the class-level names below and ``build_from_conf``.

``FactorModel`` is the other kind: the model is two factor matrices (ALS, SVD, RBMF), nothing stays resident after ``fit``, and the hooks hand out
plain tensors.
"""
from __future__ import annotations

import logging
import os
from abc import ABC, abstractmethod

import numpy as np
import scipy.sparse as sp
import torch

from .features import DeviceCSR


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


def _binary_csr(matrix, only: str) -> sp.csr_matrix:
    """the matrix as canonical CSR; ``only``: why it must be 0/1, the first clause of the refusal"""
    m = sp.csr_matrix(matrix).copy()
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    if m.nnz and bool((m.data != 1).any()):
        raise ValueError(f'{only}: the matrix has entries other than 1 (after sum_duplicates / eliminate_zeros)')
    return m


class ResidentMatrixAlgorithm(SparseMatrixBasedRecommenderAlgorithm):
    """``kwargs`` of every model: ``device``."""
    KEY = None              # the attribute that holds the model (None: not fitted) and the array of model.npz a file of this model must have
    WHAT = None             # what that is, in the state errors: 'weights'
    STORES = None           # and in the refusal of a foreign model.npz: 'the item-item weights'
    BINARY_ONLY = None      # why the matrix must be 0/1: the first clause of attach's refusal

    def __init__(self, device=None):
        super().__init__()
        self.device = torch.device(device or 'cuda')
        self.n_users = self.n_items = None
        self._matrix = None                    # the resident DeviceCSR: what _resident made of the user x item matrix

    # ---- what a model supplies ---------------------------------------------------------------------------------------------------
    def _resident(self, m: sp.csr_matrix) -> DeviceCSR:
        """the cleaned user x item matrix as the model keeps it"""
        return DeviceCSR(m)

    @abstractmethod
    def _score_rows(self, u: torch.Tensor) -> torch.Tensor:
        """-> float32 [len(u), n_items]: the score rows of the users ``u`` (int64, on the model's device)"""

    @abstractmethod
    def _npz_fields(self) -> dict:
        """what ``model.npz`` holds besides ``name``"""

    @abstractmethod
    def _read_npz(self, f):
        """take the model from an open ``model.npz`` of this model's name, or raise ``ValueError`` and leave the model as it is"""

    # ---- residency ---------------------------------------------------------------------------------------------------------------
    def to(self, device):
        self.device = torch.device(device)
        if self._matrix is not None:
            self._matrix = self._matrix.to(self.device)
        return self

    def attach(self, matrix: sp.spmatrix):
        """Make the user x item matrix resident without fitting: what a model loaded from ``model.npz`` needs before it can score."""
        m = _binary_csr(matrix, self.BINARY_ONLY)
        self.n_users, self.n_items = m.shape
        self._matrix = self._resident(m).to(self.device)
        return self

    def _need_fit(self):
        if getattr(self, self.KEY) is None:
            raise RuntimeError(f'{self.name}: no {self.WHAT}, run fit(matrix) or load_model_from_path(path)')

    def _rows(self, u: torch.Tensor) -> torch.Tensor:
        self._need_fit()
        if self._matrix is None:
            raise RuntimeError(f'{self.name}: the {self.WHAT} were loaded from model.npz, which does not hold the interactions: call '
                               f'attach(matrix) with the user x item matrix first')
        return self._score_rows(u)

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
        np.savez(os.path.join(path, 'model.npz'), **self._npz_fields(), name=np.array(self.name))
        print('Model Saved')

    def load_model_from_path(self, path: str, matrix: sp.spmatrix = None):
        with np.load(os.path.join(path, 'model.npz'), allow_pickle=False) as f:
            if 'pred_mtx' in f.files or self.KEY not in f.files:
                raise ValueError(f'{os.path.join(path, "model.npz")} is not a model of this package (it holds {f.files}): the reference '
                                 f'stores its pickled prediction matrix `pred_mtx`, this package {self.STORES}; fit the model again')
            name = str(f['name'])
            if name != self.name:
                raise ValueError(f'model.npz holds a {name}, this model is a {self.name}')
            self._read_npz(f)
        if matrix is not None:
            self.attach(matrix)
        print('Model Loaded')


class FactorModel(SparseMatrixBasedRecommenderAlgorithm):
    """The model is two float32 factor matrices, ``users_factors`` [n_users, f] and ``items_factors`` [n_items, f], and the score their dot
    product (algorithms/mf_algs.py: ALS, SVD, RBMF). Nothing of the interaction matrix is needed to score, so a loaded model needs no ``attach``,
    and both sides of the evaluation hooks are plain tensors: the fused scorers serve such a model. ``model.npz`` holds the reference's two
    fields and ``name``; a file written by the reference (no ``name``) loads as is. ``kwargs`` of every model: ``device``.

    A model writes: its constructor, ``fit`` and ``build_from_conf``; RBMF also names its two fields of ``model.npz``."""
    USERS_FIELD = 'users_factors'       # the reference's names of the two arrays in model.npz (algorithms/mf_algs.py:52-55, :127-130;
    ITEMS_FIELD = 'items_factors'       # RBMF: X and C, :197-200)

    def __init__(self, device=None):
        super().__init__()
        self.device = torch.device(device or 'cuda')
        self.users_factors = self.items_factors = None

    def to(self, device):
        self.device = torch.device(device)
        if self.users_factors is not None:
            self.users_factors, self.items_factors = self.users_factors.to(self.device), self.items_factors.to(self.device)
        return self

    def _need_fit(self):
        if self.users_factors is None or self.items_factors is None:
            raise RuntimeError(f'{self.name}: no factors, run fit(matrix) or load_model_from_path(path)')

    # ---- scoring: the hooks of evaluate_recommender_algorithm ----------------------------------------------------------------------------
    def get_user_representations(self, u_idxs: torch.Tensor) -> torch.Tensor:
        self._need_fit()
        return self.users_factors[torch.as_tensor(u_idxs).long().to(self.users_factors.device)]

    def get_item_representations(self, i_idxs: torch.Tensor) -> torch.Tensor:
        self._need_fit()
        return self.items_factors[torch.as_tensor(i_idxs).long().to(self.items_factors.device)]

    @torch.no_grad()
    def combine_user_item_representations(self, u_repr, i_repr) -> torch.Tensor:
        """[B, f] x [I, f] -> [B, I] (evaluation), [B, f] x [B, N, f] -> [B, N] (one dot product per slot)"""
        from . import ops
        return ops.score(u_repr, i_repr)

    @torch.no_grad()
    def predict(self, u_idxs: torch.Tensor, i_idxs: torch.Tensor) -> torch.Tensor:
        """algorithms/mf_algs.py:117-125: the dot products of the users' rows with the named items' rows, [batch_size, n]; taken from the
        users' full score rows, so that a score has the same bits here and in the evaluation"""
        self._need_fit()
        rows = self.combine_user_item_representations(self.get_user_representations(u_idxs), self.items_factors)
        return torch.gather(rows, 1, torch.as_tensor(i_idxs).long().to(rows.device))

    # ---- persistence -------------------------------------------------------------------------------------------------------------------
    def save_model_to_path(self, path: str):
        self._need_fit()
        np.savez(os.path.join(path, 'model.npz'), **{self.USERS_FIELD: self.users_factors.cpu().numpy(),
                                                     self.ITEMS_FIELD: self.items_factors.cpu().numpy()}, name=np.array(self.name))
        print('Model Saved')

    def load_model_from_path(self, path: str):
        with np.load(os.path.join(path, 'model.npz'), allow_pickle=False) as f:
            if 'pred_mtx' in f.files or self.USERS_FIELD not in f.files or self.ITEMS_FIELD not in f.files:
                raise ValueError(f'{os.path.join(path, "model.npz")} is not a model of this package (it holds {f.files}): the reference '
                                 f'stores its pickled prediction matrix `pred_mtx`, this package the two factor matrices; fit the model again')
            name = str(f['name']) if 'name' in f.files else self.name           # the reference's files carry no name
            if name != self.name:
                raise ValueError(f'model.npz holds a {name}, this model is a {self.name}')
            u, i = f[self.USERS_FIELD], f[self.ITEMS_FIELD]
            if u.ndim != 2 or i.ndim != 2 or u.shape[1] != i.shape[1]:
                raise ValueError(f'model.npz: factor matrices of shapes {u.shape} and {i.shape} do not belong together')
            self.users_factors = torch.from_numpy(u.astype(np.float32)).to(self.device)
            self.items_factors = torch.from_numpy(i.astype(np.float32)).to(self.device)
        print('Model Loaded')


class DenseItemModel(ResidentMatrixAlgorithm):
    """The model is one dense float32 [n_items, n_items] tensor, the public attribute named by ``KEY`` (``EASE.B``, ``P3alpha.W``);
    ``HYPER`` names the hyper-parameters (attributes) that ``model.npz`` records beside it."""
    WHAT = 'weights'
    HYPER = ()

    def __init__(self, device=None):
        super().__init__(device)
        setattr(self, self.KEY, None)

    def to(self, device):
        super().to(device)
        if getattr(self, self.KEY) is not None:
            setattr(self, self.KEY, getattr(self, self.KEY).to(self.device))
        return self

    def _weights(self) -> torch.Tensor:
        """the model on the model's device, once it fits the resident matrix"""
        w = getattr(self, self.KEY)
        if tuple(w.shape) != (self.n_items, self.n_items):
            raise ValueError(f'{self.name}: weights of shape {tuple(w.shape)} do not fit the {self.n_items} items of the matrix')
        if w.device != self.device:
            w = w.to(self.device)
            setattr(self, self.KEY, w)
        return w

    def _npz_fields(self) -> dict:
        return {self.KEY: getattr(self, self.KEY).cpu().numpy(), **{h: np.array(getattr(self, h)) for h in self.HYPER}}

    def _read_npz(self, f):
        w = f[self.KEY]
        if w.ndim != 2 or w.shape[0] != w.shape[1]:
            raise ValueError(f'model.npz: weights of shape {w.shape} are not square')
        setattr(self, self.KEY, torch.from_numpy(w.astype(np.float32)))
