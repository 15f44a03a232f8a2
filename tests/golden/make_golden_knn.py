#!/usr/bin/env python3
"""G22: UserKNN / ItemKNN (algorithms/knn_algs.py:80-118, utilities/similarities.py:18-130), generated with the REAL reference.

    PYTHONHASHSEED=0 python tests/golden/make_golden_knn.py      (build container only)

Cases: both models x {cosine, jaccard, asymmetric_cosine alpha = 0.3, tversky alpha = 0.7 beta = 0.2, sorensen_dice} x shrinkage {0, 5} x
k {5, 60} on the 50 x 40 world of make_golden.py. Per case: the reference's ``sim_mtx`` (``compute_similarity_top_k`` called as ``fit`` calls
it: indptr / indices / data) and the dense ``pred_mtx`` of ``fit``. Only data is written: g22_knn.npz + g22_knn.json.

The reference ranks with an unstable np.argsort, so which of several equal values at the k-th place it keeps is arbitrary; the comparison
rule (tests/knn_ref.py (c)) does not depend on that choice. Asserted here: at k = 60 no row is pruned; at k = 5 at most 60 % of a case's rows
are tied at the boundary (the json records the count per case).
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
from algorithms.knn_algs import ItemKNN, KNNAlgorithm, UserKNN  # noqa: E402
from utilities.similarities import SimilarityFunctionEnum, compute_similarity_top_k  # noqa: E402

import knn_ref  # noqa: E402

SIM_PARAMS = {'cosine': {}, 'jaccard': {}, 'asymmetric_cosine': {'alpha': 0.3}, 'tversky': {'alpha': 0.7, 'beta': 0.2}, 'sorensen_dice': {}}
MAX_TIED_FRACTION = 0.6

inter = sp.csr_matrix(G.make_world().inter.astype(np.float64))
arrays = {'inter': inter.toarray()}
meta = {'cases': []}
for alg in ('uknn', 'iknn'):
    for sim, params in SIM_PARAMS.items():
        for shrinkage in (0., 5.):
            for k in (5, 60):
                conf = {'alg': alg, 'k': k, 'shrinkage': shrinkage, 'sim_func_params': {'sim_func_name': sim, **params}}
                model = KNNAlgorithm.build_from_conf(conf, None)
                assert isinstance(model, UserKNN if alg == 'uknn' else ItemKNN)
                entity = inter if alg == 'uknn' else inter.T
                sim_mtx = sp.csr_matrix(compute_similarity_top_k(entity, model.sim_func, model.k, model.shrinkage, model.BLOCK_SIZE))
                model.fit(inter)
                pred = np.asarray(model.pred_mtx.todense() if sp.issparse(model.pred_mtx) else model.pred_mtx, dtype=np.float64)
                name = f'{alg}_{sim}_s{int(shrinkage)}_k{k}'
                arrays[f'{name}/sim/indptr'], arrays[f'{name}/sim/indices'] = sim_mtx.indptr.astype(np.int64), sim_mtx.indices.astype(np.int64)
                arrays[f'{name}/sim/data'], arrays[f'{name}/pred_mtx'] = sim_mtx.data.astype(np.float64), pred
                v64 = knn_ref.values(knn_ref.entity_matrix(alg, inter), sim, shrinkage, params.get('alpha'), params.get('beta'))
                n_cand = (v64 > 0).sum(axis=1)
                tied = int(knn_ref.boundary_tied(v64, k).sum())
                if k == 60:
                    assert int(n_cand.max()) < k, f'{name}: a row has {int(n_cand.max())} candidates, k = 60 prunes'
                    rows = knn_ref.fixture_rows(sim_mtx.indptr, sim_mtx.indices, sim_mtx.data)
                    assert all(len(r[0]) == c for r, c in zip(rows, n_cand)), f'{name}: the reference pruned a row'
                else:
                    assert tied <= MAX_TIED_FRACTION * len(n_cand), f'{name}: {tied} of {len(n_cand)} rows tied at the boundary'
                meta['cases'].append({'name': name, 'alg': alg, 'sim': sim, 'params': params, 'shrinkage': shrinkage, 'k': k,
                                      'model_name': model.name, 'rows': int(len(n_cand)), 'max_candidates': int(n_cand.max()),
                                      'rows_tied_at_boundary': tied})
np.savez_compressed(os.path.join(HERE, 'g22_knn.npz'), **arrays)
json.dump(meta, open(os.path.join(HERE, 'g22_knn.json'), 'w'), indent=1)
print('g22', len(arrays), max(c['rows_tied_at_boundary'] for c in meta['cases']), [(c['name'], c['rows_tied_at_boundary']) for c in meta['cases'] if c['k'] == 5])
