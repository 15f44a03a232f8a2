"""RBMF — representative-based matrix factorisation (Liu, Wei, Sun and Miao, RecSys 2011; algorithms/mf_algs.py:145-211) behind the
reference's ``SparseMatrixBasedRecommenderAlgorithm`` surface: ``n_representatives`` users are picked, ``C`` [n_items, r] holds their
interaction rows as columns, and every user is a ridge combination ``X`` [n_users, r] of them; the score is ``X C^T``.

``fit`` (``csrc/rbmf.hip``, ``csrc/svd.hip``), everything on the GPU:

    U            the r leading left singular vectors of the matrix        svd.block_iteration (the reference: scipy's svds)
    idx          r rows of U whose submatrix has locally maximal volume   ops.maxvol           (the reference: maxvolpy.maxvol.maxvol(u))
    C^T          the rows idx of the matrix, dense [n_items, r]
    K = C C^T + lam I,   M = matrix C^T                                   ops.als_gram, ops.csr_times_dense
    K = R R^T,   X = (M R^-T) R^-1                                        ops.cholesky, ops.tri_solve_rows twice

The ridge system is solved through its Cholesky factor, not through an explicit inverse (the reference's ``np.linalg.inv``; here
``ops.spd_inverse_`` and a product would have been the other way): the solve is backward stable row by row, whereas the error of a
product with a rounded ``K^-1`` grows with ``cond(K)`` and no residual vouches for it; on the test worlds (``cond(K)`` of 7 to 115)
both err alike, 3e-7 to 8e-7 of the largest element. Every kernel has a fixed operation order, so two fits with the
same ``random_state`` give the same bits.

Deliberate differences from the reference: ``maxvolpy`` is not available, so maxvol is written from the published algorithm (Goreinov,
Oseledets, Savostyanov, Tyrtyshnikov and Zamarashkin 2010) with ``tol = 1.05`` and ``max_iters = 100`` as maxvolpy's defaults are
remembered, unchecked against the package; the singular vectors come from the block iteration of ``svd.py``, not
from ARPACK; ``n_representatives <= 128``; ``lam = 0`` is refused at construction (the reference accepts it and fails on a singular
``C C^T``); a block of singular vectors of numerical rank below r is an error that asks for fewer representatives; fp32 throughout;
``model.npz`` also records ``name``.
"""
from __future__ import annotations

import logging

import numpy as np
import scipy.sparse as sp
import torch

from . import ops
from .features import DeviceCSR
from .matrix_models import FactorModel
from .svd import block_iteration, canonical_csr


class RBMF(FactorModel):
    """algorithms/mf_algs.py:145-211. ``n_representatives``: the number of representative users (1 .. 128); ``lam``: the l2 factor of the
    ridge solve (positive). ``kwargs``: ``device``, ``random_state`` (the seed of the SVD's initial block, default 0), ``tol`` and
    ``max_iters`` of maxvol (1.05 and 100), and the SVD's ``oversample`` (28), ``n_iterations`` (100, at least 1) and ``svd_tol`` (1e-5).
    ``X`` [n_users, r] and ``C`` [n_items, r] are the reference's names of ``users_factors`` and ``items_factors``. After ``fit``:
    ``representatives`` (int64 [r], the chosen users in basis order) and ``n_swaps`` (maxvol's swaps behind the LU start)."""
    USERS_FIELD = 'X'
    ITEMS_FIELD = 'C'

    def __init__(self, n_representatives: int, lam: float = 1e-2, **kwargs):
        super().__init__(kwargs.get('device'))
        r = n_representatives
        if int(r) != r or not 1 <= r <= ops.BLOCK_MAX:
            raise ValueError(f'n_representatives ({r}) has to be an integer in [1, {ops.BLOCK_MAX}]')
        if not lam > 0 or not np.isfinite(lam):
            raise ValueError(f'lam ({lam}) has to be positive: with lam = 0 the system C C^T is singular as soon as two representatives '
                             f'share their interactions')
        tol, max_iters = kwargs.get('tol', 1.05), kwargs.get('max_iters', 100)
        oversample, n_iterations, svd_tol = kwargs.get('oversample', 28), kwargs.get('n_iterations', 100), kwargs.get('svd_tol', 1e-5)
        if not (tol >= 1 and np.isfinite(tol)):
            raise ValueError(f'tol ({tol}) has to be a finite number >= 1')
        if int(max_iters) != max_iters or max_iters < 0:
            raise ValueError(f'max_iters ({max_iters}) has to be a non-negative integer')
        if int(oversample) != oversample or oversample < 0:
            raise ValueError(f'oversample ({oversample}) has to be a non-negative integer')
        if int(n_iterations) != n_iterations or n_iterations < 1:
            raise ValueError(f'n_iterations ({n_iterations}) has to be a positive integer: the representatives are rows of the singular '
                             f'vectors')
        if not svd_tol >= 0:
            raise ValueError(f'svd_tol ({svd_tol}) has to be non-negative')
        self.n_representatives = int(r)
        self.lam = lam
        self.tol, self.max_iters = float(tol), int(max_iters)
        self.oversample = min(int(oversample), ops.BLOCK_MAX - self.n_representatives)
        self.n_iterations, self.svd_tol = int(n_iterations), float(svd_tol)
        self.random_state = kwargs.get('random_state', 0)
        self.representatives = self.n_swaps = None
        self.name = 'RBMF'
        logging.info(f'Built {self.name} module \n'
                     f'- n_representatives: {self.n_representatives} \n'
                     f'- lam: {self.lam} \n')

    # the reference's attribute names (algorithms/mf_algs.py:159-160, :183-184)
    @property
    def X(self):
        return self.users_factors

    @X.setter
    def X(self, value):
        self.users_factors = value

    @property
    def C(self):
        return self.items_factors

    @C.setter
    def C(self, value):
        self.items_factors = value

    def initial_block(self, n_items: int, b: int) -> np.ndarray:
        """-> V0 [n_items, b] float32 numpy: the start of the SVD's block iteration, as ``SVDAlgorithm.initial_block``"""
        return np.random.RandomState(self.random_state).standard_normal(size=(n_items, b)).astype(np.float32)

    def fit(self, matrix: sp.spmatrix, **kwargs):
        """:param matrix: user x item sparse matrix; any finite values"""
        r = self.n_representatives
        m = canonical_csr(matrix, self.name, r, 'n_representatives')
        n_users, n_items = m.shape
        b = min(r + self.oversample, n_users, n_items)
        x = DeviceCSR(m).to(self.device)                             # X, resident during fit only
        U = block_iteration(m, self.initial_block(n_items, b), r, self.n_iterations, self.svd_tol, self.device, x=x)[0]
        idx, self.n_swaps = ops.maxvol(U[:, :r], self.tol, self.max_iters)
        self.representatives = idx
        rows = m[idx.cpu().numpy()]                                  # C = matrix[indxs], r sparse rows: a gather, done where the matrix is
        Ct = torch.from_numpy(np.ascontiguousarray(rows.toarray().T, dtype=np.float32)).to(self.device)      # C^T dense [n_items, r]
        K = ops.als_gram(Ct, float(self.lam))                        # C C^T + lam I
        M = ops.csr_times_dense(x, Ct)                               # matrix C^T
        R = ops.cholesky(K)
        Y = ops.tri_solve_rows(M, R.t().contiguous(), upper=True, out=M)
        self.users_factors, self.items_factors = ops.tri_solve_rows(Y, R, upper=False, out=Y), Ct
        return self

    @staticmethod
    def build_from_conf(conf: dict, dataset=None):
        return RBMF(conf['n_representatives'], conf['lam'])
