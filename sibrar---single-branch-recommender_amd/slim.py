"""SLIM — Sparse Linear Methods (Ning and Karypis, ICDM 2011; algorithms/linear_algs.py:15-127) behind the reference's
``SparseMatrixBasedRecommenderAlgorithm`` surface.

The reference fits one sklearn ``ElasticNet`` (``positive=True``, ``fit_intercept=False``, ``selection="random"``, ``tol=1e-4``) per item
in a CPU process pool, on the users x items matrix with the target item's column zeroed. Each of these problems depends on the matrix
only through the Gram matrix ``G = X^T X``, so ``fit(matrix)`` keeps the interaction matrix resident as CSR, counts ``G`` into one dense
float32 [n_items, n_items] buffer (``ops.gram_dense``: exact) and solves all columns from it on the chip (``ops.slim_weights``: one
workgroup per column, cyclic coordinate descent with the residual in LDS, csrc/slim.hip) with ``l1 = n_users alpha l1_ratio`` and
``l2 = n_users alpha (1 - l1_ratio)``. The dense float32 result is the model, ``self.W``: ``W[k, j]`` is the weight of item k for target j.
The reference's ``pred_mtx`` (users x items) is never built: score rows are made per user chunk by ``ops.csr_rows_times_dense`` —
``matrix[u] @ W`` (linear_algs.py:59-61).

Full-catalogue evaluation goes through the hooks ``evaluate_recommender_algorithm`` already calls, exactly as for EASE: the item side is a
1-tuple (the item ids), which takes the ``fp32`` route.

Deliberate differences from the reference: the coordinates are taken in ascending cyclic order (the reference: random order; with
``l2 > 0`` the optimum is unique and the order only changes the path to it); a column stops after the sweep whose largest weight change is at
most ``tol`` times the largest weight, sklearn's first test, and sklearn's dual-gap test behind it is not reproduced; everything is fp32 (the
reference: float64); the interaction data must be 0/1; ``W`` is dense, and the number of items is limited by the LDS a column's residual
needs (``ops.SLIM_MAX_ITEMS``); ``model.npz`` holds ``W``, not ``pred_mtx``, so a loaded model needs the interaction matrix again
(``attach``). Columns that reach ``max_iter`` unconverged are counted in a ``logging.warning`` (sklearn raises a ``ConvergenceWarning``
there, which the reference silences); ``n_iter_`` keeps the sweeps per column of the last ``fit``: a record of that run, not part of the
model — ``to()`` does not move it and ``model.npz`` does not hold it (a loaded model has ``n_iter_ = None``).
"""
from __future__ import annotations

import logging

import scipy.sparse as sp

from . import ops
from .matrix_models import DenseItemModel


class SLIM(DenseItemModel):
    """algorithms/linear_algs.py:15-127. ``alpha``: a + b, ``l1_ratio``: a / (a + b) for the multipliers a, b of the L1 and L2 penalties;
    ``max_iter``: the most sweeps per item. ``kwargs``: ``device``, ``tol`` (1e-4, the reference's, linear_algs.py:78)."""
    KEY, HYPER = 'W', ('alpha', 'l1_ratio', 'max_iter', 'tol')           # self.W, the model: float32 [n_items, n_items]
    STORES = 'the item-item weights'
    BINARY_ONLY = 'SLIM: the elastic nets are solved from the Gram matrix, which is counted as integers for 0/1 interaction data only'

    def __init__(self, alpha: float, l1_ratio: float, max_iter: int, **kwargs):
        super().__init__(kwargs.get('device'))
        tol = kwargs.get('tol', 1e-4)
        if not alpha >= 0:
            raise ValueError(f'alpha={alpha!r} must not be negative')
        if not 0 <= l1_ratio <= 1:
            raise ValueError(f'l1_ratio={l1_ratio!r} outside [0, 1]')
        if not (int(max_iter) == max_iter and max_iter >= 1):
            raise ValueError(f'max_iter={max_iter!r} must be an integer >= 1')
        if not tol >= 0:
            raise ValueError(f'tol={tol!r} must not be negative')
        self.alpha, self.l1_ratio, self.max_iter, self.tol = alpha, l1_ratio, int(max_iter), tol
        self.n_iter_ = None                    # int32 [n_items] after fit: the sweeps per column, negative where max_iter was reached
        self.name = 'SLIM'
        logging.info(f'Built {self.name} module \n- alpha: {self.alpha} \n- l1_ratio: {self.l1_ratio} \n- max_iter: {self.max_iter} \n')

    def penalties(self, n_users: int):
        """(l1, l2) of the Gram form: sklearn's alpha l1_ratio and alpha (1 - l1_ratio) times the number of samples, in double"""
        return float(n_users) * float(self.alpha) * float(self.l1_ratio), float(n_users) * float(self.alpha) * (1. - float(self.l1_ratio))

    def fit(self, matrix: sp.spmatrix, **kwargs):
        """:param matrix: user x item sparse matrix"""
        self.attach(matrix)
        self.W = self.n_iter_ = None
        G = ops.gram_dense(self._matrix, 0.)                              # the design matrix enters through X^T X only
        l1, l2 = self.penalties(self.n_users)
        self.W, self.n_iter_ = ops.slim_weights(G, l1, l2, self.max_iter, self.tol)           # linear_algs.py:65-112
        del G
        late = int((self.n_iter_ < 0).sum())
        if late:
            logging.warning(f'{self.name}: {late} of {self.n_items} columns did not converge in max_iter={self.max_iter} sweeps (tol={self.tol})')
        return self

    def _score_rows(self, u):
        return ops.csr_rows_times_dense(self._matrix, u, self._weights())  # linear_algs.py:59-61

    @staticmethod
    def build_from_conf(conf: dict, dataset=None):
        return SLIM(conf['alpha'], conf['l1_ratio'], conf['max_iter'])
