#!/usr/bin/env python3
"""G23: EASE (algorithms/linear_algs.py:130-175), generated with the REAL reference.

    PYTHONHASHSEED=0 python tests/golden/make_golden_ease.py      (build container only)

Cases: lam in {1, 10, 500.7} on the 50 x 40 world of make_golden.py (500.7 reaches the diagonal as 500). Per case: the dense ``pred_mtx`` of the
reference's ``fit`` and the weights ``B``, recomputed here as ``fit`` computes them (it keeps only ``pred_mtx``), both float64. Only data is
written: g23_ease.npz + g23_ease.json.

Asserted here: ``matrix @ B`` is the reference's ``pred_mtx`` bit for bit; at most 10 % of the users are left out of the top-10 comparison by the
near-tie rule of tests/ease_ref.py (the json records the count per case, with the fp32 yardstick ``e_ref`` it was taken at).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402  (installs the import placeholders, asserts PYTHONHASHSEED=0)

import scipy.sparse as sp  # noqa: E402
from algorithms.linear_algs import EASE  # noqa: E402

import ease_ref as R  # noqa: E402

inter = sp.csr_matrix(G.make_world().inter.astype(np.float64))
arrays = {'inter': inter.toarray()}
meta = {'cases': []}
for lam in R.LAMS:
    model = EASE.build_from_conf({'lam': lam}, None)
    model.fit(inter)
    pred = np.asarray(model.pred_mtx, dtype=np.float64)
    b = R.weights(np.linalg.inv(R.gram(inter, model.lam)))
    assert np.array_equal(np.asarray(inter @ b), pred), f'lam={lam}: the recomputed weights do not give the reference pred_mtx'
    name = f'lam{int(lam)}'
    arrays[f'{name}/B'], arrays[f'{name}/pred_mtx'] = b, pred
    err_b = R.e_ref_weights(R.gram(inter, lam))
    left_out = int((~R.countable_users(pred, inter, err_b)).sum())
    assert left_out <= R.MAX_LEFT_OUT * inter.shape[0], f'{name}: {left_out} of {inter.shape[0]} users are near-tied at the 10th place'
    meta['cases'].append({'name': name, 'lam': lam, 'diag': int(lam), 'model_name': model.name, 'users': int(inter.shape[0]),
                          'e_ref_weights': err_b, 'users_left_out': left_out})
np.savez_compressed(os.path.join(HERE, 'g23_ease.npz'), **arrays)
json.dump(meta, open(os.path.join(HERE, 'g23_ease.json'), 'w'), indent=1)
print('g23', len(arrays), [(c['name'], c['e_ref_weights'], c['users_left_out']) for c in meta['cases']])
