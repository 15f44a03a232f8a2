#!/usr/bin/env python3
"""G24: P3alpha (algorithms/graph_algs.py:9-88), generated with the REAL reference.

    PYTHONHASHSEED=0 python tests/golden/make_golden_p3alpha.py      (build container only)

Cases: alpha in {1.9, 1.0, 0.5} on the 50 x 40 world of make_golden.py and, since that world has no user and no item without
interactions, on a copy of it with one user and one item zeroed ('empty/...'). Per case: the dense float64 ``pred_mtx`` of the reference's
``fit``. Only data is written: g24_p3alpha.npz (the two interaction matrices and ``pred_mtx`` per case) + g24_p3alpha.json.

Asserted here: the three-factor product of tests/p3alpha_ref.py meets the reference's ``pred_mtx`` to 1e-12 relative; empty rows and
columns are zeros, not NaN; at most 10 % of the users are left out of the top-10 comparison by the near-tie rule of tests/p3alpha_ref.py
(the json records the count per case).
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402  (installs the import placeholders, asserts PYTHONHASHSEED=0)

import scipy.sparse as sp  # noqa: E402
from algorithms.graph_algs import P3alpha  # noqa: E402

import p3alpha_ref as R  # noqa: E402

EMPTY_USER, EMPTY_ITEM = 11, 29

dense = G.make_world().inter.toarray().astype(np.float64)
matrices = {'inter': dense}
if dense.sum(axis=1).min() > 0 or dense.sum(axis=0).min() > 0:
    e = dense.copy()
    e[EMPTY_USER] = 0
    e[:, EMPTY_ITEM] = 0
    matrices['inter_empty'] = e
arrays = dict(matrices)
meta = {'cases': []}
for key, d in matrices.items():
    inter = sp.csr_matrix(d)
    for alpha in R.ALPHAS:
        model = P3alpha.build_from_conf({'alpha': alpha}, None)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                                    # 1 / 0 of an empty user or item: a numpy warning only
            model.fit(inter)
        pred = np.asarray(model.pred_mtx.toarray(), dtype=np.float64)
        assert np.isfinite(pred).all(), f'{key} alpha={alpha}: the reference gives non-finite scores'
        _, pred64 = R.fit64(inter, alpha)
        assert np.abs(pred64 - pred).max() <= 1e-12 * np.abs(pred).max(), f'{key} alpha={alpha}: the three-factor product misses pred_mtx'
        assert np.array_equal(pred64 == 0, pred == 0)
        name = ('' if key == 'inter' else 'empty/') + f'a{alpha}'
        arrays[f'{name}/pred_mtx'] = pred
        left_out = int((~R.countable_users(pred, inter, alpha)).sum())
        assert left_out <= R.MAX_LEFT_OUT * inter.shape[0], f'{name}: {left_out} of {inter.shape[0]} users are near-tied at the 10th place'
        meta['cases'].append({'name': name, 'matrix': key, 'alpha': alpha, 'model_name': model.name, 'users': int(inter.shape[0]),
                              'empty_users': int((d.sum(axis=1) == 0).sum()), 'empty_items': int((d.sum(axis=0) == 0).sum()),
                              'users_left_out': left_out})
np.savez_compressed(os.path.join(HERE, 'g24_p3alpha.npz'), **arrays)
json.dump(meta, open(os.path.join(HERE, 'g24_p3alpha.json'), 'w'), indent=1)
print('g24', len(arrays), [(c['name'], c['users_left_out']) for c in meta['cases']])
