#!/usr/bin/env python3
"""G26: SLIM (algorithms/linear_algs.py:15-127), generated with the REAL reference.

    PYTHONHASHSEED=0 python tests/golden/make_golden_slim.py      (build container only)

Cases: (alpha, l1_ratio, max_iter) in tests/slim_ref.py's PARAMS on the 50 x 40 world of make_golden.py. Per case: the dense float64
``pred_mtx`` of the reference's ``fit``; the reference's weights ``W_ref``, the triplets of one in-process ``SLIM.work`` call over all
columns (``fit`` keeps only ``pred_mtx``); and ``W_opt``, the optimum by the float64 restatement of tests/slim_ref.py at tol = 1e-12.
Only data is written: g26_slim.npz + g26_slim.json.

``multiprocessing.cpu_count`` is set to 2 before ``fit``: the reference's ``generate_slices`` cuts ``n_items // cores`` columns per task,
and with more cores than items that length is 0 and its loop never ends. numpy's global generator is seeded before every reference run:
sklearn's ``selection="random"`` draws from it (``random_state=None``), in ``fit``'s pool workers from their copy of it.

Asserted here: per column, the reference's objective (times n) is within 1e-4 G_jj of the optimum's — what its stopping rule,
gap <= tol y.y, promises once it has converged; ``inter @ W_ref`` meets ``pred_mtx`` to 1e-3 (two random runs); the KKT residual of
``W_opt`` is at most 1e-8; at most 10 % of the users are left out of the top-10 comparison by the near-tie rule of tests/slim_ref.py
(the json records the count per case, with ``max |W_ref - W_opt|`` and the fp32 yardstick it was taken at).
"""
import json
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402  (installs the import placeholders, asserts PYTHONHASHSEED=0)

import scipy.sparse as sp  # noqa: E402
from algorithms.linear_algs import SLIM  # noqa: E402

import slim_ref as R  # noqa: E402

multiprocessing.cpu_count = lambda: 2

if __name__ == '__main__':
    dense = G.make_world().inter.toarray().astype(np.float64)
    assert set(np.unique(dense)) == {0., 1.}
    inter = sp.csr_matrix(dense)
    n, m = inter.shape
    g = R.gram(inter)
    arrays = {'inter': dense}
    meta = {'cases': []}
    for alpha, l1_ratio, max_iter in R.PARAMS:
        model = SLIM.build_from_conf({'alpha': alpha, 'l1_ratio': l1_ratio, 'max_iter': max_iter}, None)
        np.random.seed(26)
        model.fit(inter)
        pred = np.asarray(model.pred_mtx, dtype=np.float64)
        np.random.seed(26)
        rows, cols, data = SLIM.work([0, m, sp.csc_matrix(inter), alpha, l1_ratio, max_iter])
        w_ref = np.asarray(sp.csr_matrix((data, (rows, cols)), shape=(m, m)).todense(), dtype=np.float64)
        assert np.abs(np.asarray(inter @ w_ref) - pred).max() <= 1e-3, 'two runs of the reference differ by more than its tolerance'
        l1, l2 = R.penalties(n, alpha, l1_ratio)
        w_opt, n_iter, _ = R.cd(g, l1, l2, 100000, 1e-12)
        assert (n_iter > 0).all() and (np.diag(w_opt) == 0).all() and (np.diag(w_ref) == 0).all() and (w_ref >= 0).all()
        kkt = R.kkt_all(g, w_opt, l1, l2)
        assert kkt <= 1e-8, kkt
        excess = max((R.objective(g, j, w_ref[:, j], l1, l2) - R.objective(g, j, w_opt[:, j], l1, l2)) / g[j, j] for j in range(m))
        assert excess <= R.OBJ_TOL, f'the reference ends {excess} G_jj above the optimum'
        e, _, _ = R.e_ref(g, l1, l2, max_iter)
        w_gap = float(np.abs(w_ref - w_opt).max())
        left_out = int((~R.countable_users(pred, np.asarray(inter @ w_opt), inter, R.FACTOR * e)).sum())
        assert left_out <= R.MAX_LEFT_OUT * n, f'{left_out} of {n} users are near-tied at the 10th place'
        name = R.case_name(alpha, l1_ratio)
        arrays[f'{name}/pred_mtx'], arrays[f'{name}/W_ref'], arrays[f'{name}/W_opt'] = pred, w_ref, w_opt
        meta['cases'].append({'name': name, 'alpha': alpha, 'l1_ratio': l1_ratio, 'max_iter': max_iter, 'model_name': model.name,
                              'users': int(n), 'max_w_ref_minus_w_opt': w_gap, 'e_ref': e, 'objective_excess_over_gjj': float(excess),
                              'kkt_w_opt': kkt, 'nnz_w_opt': int((w_opt > 0).sum()), 'users_left_out': left_out})
    np.savez_compressed(os.path.join(HERE, 'g26_slim.npz'), **arrays)
    json.dump(meta, open(os.path.join(HERE, 'g26_slim.json'), 'w'), indent=1)
    print('g26', len(arrays), [(c['name'], c['max_w_ref_minus_w_opt'], c['e_ref'], c['users_left_out']) for c in meta['cases']])
