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

import scipy.sparse as sp

from . import ops
from .matrix_models import DenseItemModel, SparseMatrixBasedRecommenderAlgorithm      # noqa: F401


class EASE(DenseItemModel):
    """algorithms/linear_algs.py:130-175. ``lam``: the L2 regularisation; the diagonal gets ``int(lam)`` (:153). ``kwargs``: ``device``."""
    KEY, HYPER = 'B', ('lam',)             # self.B, the model: float32 [n_items, n_items]
    STORES = 'the item-item weights'
    BINARY_ONLY = ('EASE: the Gram matrix is counted with integer atomics, and its entries are integer counts for 0/1 interaction '
                   'data only')

    def __init__(self, lam, **kwargs):
        super().__init__(kwargs.get('device'))
        if int(lam) < 1:
            raise ValueError(f'lam={lam!r}: the diagonal gets int(lam) = {int(lam)} (algorithms/linear_algs.py:153), and below 1 the Gram matrix '
                             f'may be singular; the fp32 sweep needs a positive definite matrix (a deliberate difference from the reference)')
        self.lam = lam
        self.name = 'EASE'
        logging.info(f'Built {self.name} module \n- lam: {self.lam} ')

    def fit(self, matrix: sp.spmatrix, **kwargs):
        """:param matrix: user x item sparse matrix"""
        self.attach(matrix)
        self.B = None
        G = ops.gram_dense(self._matrix, float(int(self.lam)))            # linear_algs.py:150-153
        self.B = ops.ease_weights_(ops.spd_inverse_(G))                  # :155-158, both in place
        return self

    def _score_rows(self, u):
        return ops.csr_rows_times_dense(self._matrix, u, self._weights())  # :160

    @staticmethod
    def build_from_conf(conf: dict, dataset=None):
        return EASE(conf['lam'])
