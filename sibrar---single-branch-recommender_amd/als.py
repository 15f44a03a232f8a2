"""ALS — implicit-feedback alternating least squares (Hu, Koren and Volinsky, ICDM 2008; algorithms/mf_algs.py:69-142) behind the
reference's ``SparseMatrixBasedRecommenderAlgorithm`` surface.

The reference wraps the ``implicit`` library. Its confidence convention is kept ("alpha: the weights given to the positive examples"):
an observed entry has confidence ``c = alpha * r_ui``, every other entry ``c = 1``, and the preference is 1 for observed entries, 0
elsewhere. A half-sweep recomputes every row of one factor matrix from the other, ``Y``:

    A_r = (Y^T Y + regularization I) + sum_{i in S} (alpha r_i - 1) y_i y_i^T,   b_r = sum_{i in S} alpha r_i y_i,   x_r = A_r^-1 b_r

``ops.als_gram`` computes the shared part once per half-sweep and ``ops.als_solve_rows`` assembles, factors (Cholesky, in LDS) and solves
one system per row (``csrc/als.hip``); both are fixed-order, so two fits with the same ``random_state`` give the same bits. ``fit`` keeps X
and X^T resident as CSR only while it runs. The model is ``users_factors`` and ``items_factors`` (float32 device tensors); the hooks hand
them out as plain tensors, so ``evaluate_recommender_algorithm`` serves ALS on all three scorer routes (``factors`` of 64 and 128 take
the fused kernels).

Deliberate differences from the reference: every row's system is solved exactly, where ``implicit`` runs three warm-started conjugate
gradient steps by default; the factors start as float32 ``RandomState(random_state).uniform(-0.5 / f, 0.5 / f)``, users first (``implicit``
draws its own); ``factors <= 128``; ``use_gpu=False`` is refused (no CPU fallback in this package); ``model.npz`` also records ``name``.
Everything is fp32: the Cholesky factorisation needs ``regularization`` well above ``f * 2^-24 * ||A||`` and says so when a pivot fails.
"""
from __future__ import annotations

import logging
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp
import torch

from . import ops
from .features import DeviceCSR
from .matrix_models import FactorModel, SparseMatrixBasedRecommenderAlgorithm      # noqa: F401


class AlternatingLeastSquare(FactorModel):
    """algorithms/mf_algs.py:69-142. ``alpha``: the confidence of a positive example is ``alpha * r``; ``factors``: the embedding size
    (1 .. 128); ``regularization``: the l2 factor; ``n_iterations``: full sweeps (users, then items). ``kwargs``: ``device``,
    ``random_state`` (the seed of the initial factors, default 0)."""

    def __init__(self, alpha: float, factors: int, regularization: float, n_iterations: int, use_gpu: bool = True, **kwargs):
        super().__init__(kwargs.get('device'))
        if not use_gpu:
            raise ValueError('use_gpu=False: this package has no CPU fallback, ALS runs on the GPU only')
        if int(factors) != factors or not 1 <= factors <= ops.BLOCK_MAX:
            raise ValueError(f'factors ({factors}) has to be an integer in [1, {ops.BLOCK_MAX}]')
        if not alpha > 0 or not np.isfinite(alpha):
            raise ValueError(f'alpha ({alpha}) has to be positive')
        if not regularization > 0 or not np.isfinite(regularization):
            raise ValueError(f'regularization ({regularization}) has to be positive')
        if int(n_iterations) != n_iterations or n_iterations < 0:
            raise ValueError(f'n_iterations ({n_iterations}) has to be a non-negative integer')
        self.alpha = alpha
        self.factors = int(factors)
        self.regularization = regularization
        self.n_iterations = int(n_iterations)
        self.use_gpu = use_gpu
        self.random_state = kwargs.get('random_state', 0)
        self.name = 'AlternatingLeastSquare'
        logging.info(f'Built {self.name} module \n'
                     f'- alpha: {self.alpha} \n'
                     f'- factors: {self.factors} \n'
                     f'- regularization: {self.regularization} \n'
                     f'- n_iterations: {self.n_iterations} \n'
                     f'- use_gpu: {self.use_gpu} \n')

    def initial_factors(self, n_users: int, n_items: int):
        """-> (users [n_users, f], items [n_items, f]) float32 numpy: one ``RandomState(random_state)`` stream, users first"""
        rng, f = np.random.RandomState(self.random_state), self.factors
        return (rng.uniform(-0.5 / f, 0.5 / f, size=(n_users, f)).astype(np.float32),
                rng.uniform(-0.5 / f, 0.5 / f, size=(n_items, f)).astype(np.float32))

    def fit(self, matrix: sp.spmatrix, **kwargs):
        """:param matrix: user x item sparse matrix; its values are the ``r_ui`` (positive and finite)"""
        m = sp.csr_matrix(matrix).copy()
        m.sum_duplicates()
        m.eliminate_zeros()
        m.sort_indices()
        if m.nnz and not bool((np.isfinite(m.data) & (m.data > 0)).all()):
            raise ValueError('AlternatingLeastSquare: the matrix has negative or non-finite entries (after sum_duplicates / eliminate_zeros); '
                             'the confidence alpha * r is stated for positive values')
        n_users, n_items = m.shape
        users, items = (torch.from_numpy(a) for a in self.initial_factors(n_users, n_items))
        if self.n_iterations:
            x = DeviceCSR(m).to(self.device)                         # X, resident during fit only
            t_indptr, t_indices, t_data = x.transposed()
            xt = SimpleNamespace(shape=(n_items, n_users), indptr=t_indptr, indices=t_indices, data=t_data)      # X^T, made on the device
        users, items = users.to(self.device), items.to(self.device)
        for _ in range(self.n_iterations):
            users = ops.als_solve_rows(x, items, ops.als_gram(items, self.regularization), self.alpha)
            items = ops.als_solve_rows(xt, users, ops.als_gram(users, self.regularization), self.alpha)
        self.users_factors, self.items_factors = users, items
        return self

    @staticmethod
    def build_from_conf(conf: dict, dataset=None):
        return AlternatingLeastSquare(conf['alpha'], conf['factors'], conf['regularization'], conf['n_iterations'], conf['use_gpu'])
