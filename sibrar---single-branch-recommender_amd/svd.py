"""SVD — the truncated singular value decomposition of the user x item matrix (algorithms/mf_algs.py:14-66) behind the reference's
``SparseMatrixBasedRecommenderAlgorithm`` surface: ``users_factors = U_k diag(s_k)``, ``items_factors = V_k``, the score their dot product.

The reference calls ``scipy.sparse.linalg.svds`` (ARPACK, on the CPU). Here a block ``V`` [n_items, b] of ``b = min(factors + oversample,
n_users, n_items) <= 128`` columns is iterated on the GPU, with a Rayleigh-Ritz step on every half-iteration (``csrc/svd.hip``):

    Y = X V,   U = orth(Y);      Z = X^T U,   (V, s, W) = orth(Z),   U <- U W

where ``orth(Y) = Y W diag(1 / s)`` with ``Y^T Y = W diag(lam) W^T`` (``ops.gram``, then ``ops.sym_eig``: Jacobi on the Gram matrix, which
is graded and nearly diagonal from the second iteration on, the case in which Jacobi keeps relative accuracy), ``lam`` descending and
``s = sqrt(max(lam, tiny))``. The next iteration's ``Y = X V`` gives the residuals ``||Y[:, i] - s_i U[:, i]||_2``, i < factors, at no
extra product: the iteration stops when the largest is ``<= tol * s_0``, or after ``n_iterations``. Every kernel has a fixed operation
order, so two fits with the same ``random_state`` give the same bits. X and X^T are resident as CSR only while ``fit`` runs.

Deliberate differences from the reference: the components come in descending order of the singular value (``svds`` returns them
ascending) and every right singular vector's sign is fixed by its rotation's largest component, not by ARPACK's start vector (scores do
not depend on either); block iteration instead of ARPACK's Lanczos process, from float32 ``RandomState(random_state).standard_normal``;
a fit that has not met ``tol`` logs a warning with its residual where ARPACK raises; ``factors <= 128``, and ``factors == min(n_users,
n_items)`` is fine (``svds`` needs ``k < min``); fp32 throughout; ``model.npz`` also records ``name``.
"""
from __future__ import annotations

import logging
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp
import torch

from . import ops
from .features import DeviceCSR
from .matrix_models import FactorModel


def canonical_csr(matrix, name: str, f: int, what: str) -> sp.csr_matrix:
    """the matrix as canonical CSR, refused when it has fewer than ``f`` singular triplets (``what``: the parameter's name) or a
    non-finite entry"""
    m = sp.csr_matrix(matrix).copy()
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    n_users, n_items = m.shape
    if f > min(n_users, n_items):
        raise ValueError(f'{name}: {what} ({f}) exceeds min(n_users, n_items) = {min(n_users, n_items)}: the matrix has no more '
                         f'singular triplets')
    if m.nnz and not bool(np.isfinite(m.data).all()):
        raise ValueError(f'{name}: the matrix has non-finite entries')
    return m


def _orth(Y):
    """(Y W diag(1 / s) in place of Y, s, W) with Y^T Y = W diag(lam) W^T"""
    lam, W = ops.sym_eig(ops.gram(Y))
    Y, s = ops.rotate_cols(Y, W, lam, out=Y)
    return Y, s, W


def block_iteration(m: sp.csr_matrix, V0: np.ndarray, f: int, n_iterations: int, tol: float, device, x=None):
    """The block subspace iteration of the module's header on the canonical CSR ``m`` from the start ``V0`` [n_items, b] ->
    ``(U [n_users, b], s [b], V [n_items, b], Y = X V, iterations run, residual history)``: the left singular vectors themselves (RBMF
    selects its representatives among their rows), the singular values descending and the right singular vectors; ``U`` and ``s`` are
    None when ``n_iterations`` is 0. The iteration stops when the largest residual of the first ``f`` triplets is ``<= tol * s_0``.
    ``x``: X already resident (a ``DeviceCSR`` on ``device``); it is made here, for the time of the call, when None."""
    n_users, n_items = m.shape
    if x is None:
        x = DeviceCSR(m).to(device)                                  # X, resident during fit only
    t_indptr, t_indices, t_data = x.transposed()
    xt = SimpleNamespace(shape=(n_items, n_users), indptr=t_indptr, indices=t_indices, data=t_data)      # X^T, made on the device
    V, _, _ = _orth(torch.from_numpy(V0).to(device))
    U = s = None
    history = []
    for it in range(n_iterations + 1):
        Y = ops.csr_times_dense(x, V)
        if it:
            history.append(float(ops.col_residual(Y, U, s, f).max()))
            if history[-1] <= tol * float(s[0]):
                break
        if it == n_iterations:
            break
        U, _, _ = _orth(Y)
        V, s, W = _orth(ops.csr_times_dense(xt, U))
        ops.rotate_cols(U, W, out=U)
    return U, s, V, Y, it, history


class SVDAlgorithm(FactorModel):
    """algorithms/mf_algs.py:14-66. ``factors``: the number of singular triplets kept (1 .. 128). ``kwargs``: ``device``, ``random_state``
    (the seed of the initial block, default 0), ``oversample`` (extra columns of the iterated block, default 28, clipped so that the block
    has at most 128), ``n_iterations`` (the cap, default 100) and ``tol`` (the largest residual of a kept triplet, relative to the largest
    singular value, default 1e-5; DESIGN.md §4.21 has the floors both rest on). After ``fit``: ``singular_values`` (float32 [factors],
    descending), ``n_iterations_run``, ``residual`` (the largest residual, absolute) and ``residual_history`` (one per iteration)."""

    def __init__(self, factors: int = 100, **kwargs):
        super().__init__(kwargs.get('device'))
        if int(factors) != factors or not 1 <= factors <= ops.BLOCK_MAX:
            raise ValueError(f'factors ({factors}) has to be an integer in [1, {ops.BLOCK_MAX}]')
        oversample, n_iterations, tol = kwargs.get('oversample', 28), kwargs.get('n_iterations', 100), kwargs.get('tol', 1e-5)
        if int(oversample) != oversample or oversample < 0:
            raise ValueError(f'oversample ({oversample}) has to be a non-negative integer')
        if int(n_iterations) != n_iterations or n_iterations < 0:
            raise ValueError(f'n_iterations ({n_iterations}) has to be a non-negative integer')
        if not tol >= 0:
            raise ValueError(f'tol ({tol}) has to be non-negative')
        self.factors = int(factors)
        self.oversample = min(int(oversample), ops.BLOCK_MAX - self.factors)
        self.n_iterations = int(n_iterations)
        self.tol = float(tol)
        self.random_state = kwargs.get('random_state', 0)
        self.singular_values = self.n_iterations_run = self.residual = self.residual_history = None
        self.name = 'SVDAlgorithm'
        logging.info(f'Built {self.name} module \n'
                     f'- factors: {self.factors} \n')

    def initial_block(self, n_items: int, b: int) -> np.ndarray:
        """-> V0 [n_items, b] float32 numpy: ``RandomState(random_state).standard_normal``, before it is orthonormalised"""
        return np.random.RandomState(self.random_state).standard_normal(size=(n_items, b)).astype(np.float32)

    _orth = staticmethod(_orth)          # (tools/time_svd.py times one iteration by hand)

    def fit(self, matrix: sp.spmatrix, **kwargs):
        """:param matrix: user x item sparse matrix; any finite values"""
        m = canonical_csr(matrix, self.name, self.factors, 'factors')
        n_users, n_items = m.shape
        f = self.factors
        b = min(f + self.oversample, n_users, n_items)
        U, s, V, Y, self.n_iterations_run, self.residual_history = block_iteration(m, self.initial_block(n_items, b), f, self.n_iterations,
                                                                                   self.tol, self.device)
        history = self.residual_history
        if U is None:                                                # no iteration: the orthonormalised start and its projection
            self.users_factors, self.items_factors = Y[:, :f].contiguous(), V[:, :f].contiguous()
            self.singular_values, self.residual = torch.sqrt(torch.diagonal(ops.gram(Y))[:f]), float('inf')
            return self
        self.residual = history[-1]
        if not self.residual <= self.tol * float(s[0]):
            logging.warning(f'{self.name}: the largest residual of the {f} triplets is {self.residual:.3e} = {self.residual / float(s[0]):.3e} '
                            f'* s_0 after {self.n_iterations_run} iterations, above tol = {self.tol:g}: the spectrum has no gap behind '
                            f'the block of {b} columns; raise n_iterations or oversample')
        self.singular_values = s[:f].clone()
        self.users_factors, self.items_factors = (U[:, :f] * s[:f]).contiguous(), V[:, :f].contiguous()
        return self

    @staticmethod
    def build_from_conf(conf: dict, dataset=None):
        return SVDAlgorithm(conf['n_factors'])
