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

import scipy.sparse as sp

from . import ops
from .matrix_models import DenseItemModel, SparseMatrixBasedRecommenderAlgorithm      # noqa: F401


class P3alpha(DenseItemModel):
    """algorithms/graph_algs.py:9-88. ``alpha``: the elementwise power of the walk probabilities (:68). ``kwargs``: ``device``."""
    KEY, HYPER = 'W', ('alpha',)           # self.W, the model: float32 [n_items, n_items]
    STORES = 'the item-item matrix of the walk'
    BINARY_ONLY = 'P3alpha: the walk is computed from entry counts, which are the degrees for 0/1 interaction data only'

    def __init__(self, alpha: float = 1.9, **kwargs):
        super().__init__(kwargs.get('device'))
        if alpha < 0:
            raise ValueError(f'Alpha ({alpha}) has to be greater or equal than 0')              # graph_algs.py:18 asserts
        if alpha == 0:
            raise ValueError('alpha=0: the reference accepts it at construction and its fit fails (scipy refuses a zero power, '
                             'algorithms/graph_algs.py:68); refused here at once (a deliberate difference from the reference)')
        self.alpha = alpha
        self.name = 'P3alpha'
        logging.info(f'Built {self.name} module \n- alpha: {self.alpha}')

    def fit(self, matrix: sp.spmatrix, **kwargs):
        """:param matrix: user x item sparse matrix"""
        self.attach(matrix)
        self.W = None
        self.W = ops.p3_walk_dense(self._matrix)                          # graph_algs.py:35-59
        return self

    def _score_rows(self, u):
        return ops.p3_score_rows(self._matrix, u, self._weights(), self.alpha)     # graph_algs.py:59-68

    @staticmethod
    def build_from_conf(conf: dict, dataset=None):
        return P3alpha(alpha=conf['alpha'])
