#!/usr/bin/env python3
"""G25: ItemFeatureKNN (algorithms/knn_algs.py:121-140, utilities/similarities.py:18-61, :86-93), generated with the REAL reference.

    PYTHONHASHSEED=0 python tests/golden/make_golden_ifknn.py      (build container only)

World: the 50 x 40 interactions of make_golden.py; features: default_rng(SEED) normal [40, 24] with row 7 all zero and row 31 a copy of
row 12. Cases: the signed features with shrinkage 0 and |features| with shrinkage {0, 5}, each at k {5, 60}. Per case: the reference's
``sim_mtx`` (``compute_similarity_top_k`` called as ``fit`` calls it: indptr / indices / data, its explicit zeros kept) and the dense
``pred_mtx`` of ``fit``. Only data is written: g25_ifknn.npz + g25_ifknn.json.

The reference ranks with an unstable np.argsort, so which of several equal values at the k-th place it keeps is arbitrary; the comparison
rule (tests/ifknn_ref.py (d)) does not depend on that choice. Asserted here: at k = 60 no non-zero row is pruned; at k = 5 at most 10 % of a
case's rows are tied at the boundary (the json records the count per case; the duplicated row ties its two copies everywhere else, which is
why the seed is chosen); no pair has a float64 |dot| below 1e-9 sum_k |x_k y_k| other than exact zeros.
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
from algorithms.knn_algs import ItemFeatureKNN, KNNAlgorithm  # noqa: E402
from utilities.similarities import compute_similarity_top_k  # noqa: E402

import ifknn_ref  # noqa: E402

SEED = int(os.environ.get('G25_SEED', '2'))
MAX_TIED_FRACTION = 0.1
ZERO_ROW, DUP_ROW, DUP_OF = 7, 31, 12

inter = sp.csr_matrix(G.make_world().inter.astype(np.float64))
n_items = inter.shape[1]
features = np.random.default_rng(SEED).normal(size=(n_items, 24))
features[ZERO_ROW] = 0.
features[DUP_ROW] = features[DUP_OF]
arrays = {'inter': inter.toarray(), 'features': features}
meta = {'seed': SEED, 'zero_row': ZERO_ROW, 'dup_row': DUP_ROW, 'dup_of': DUP_OF, 'cases': []}
for which, shrinkages in (('signed', (0.,)), ('abs', (0., 5.))):
    f = np.abs(features) if which == 'abs' else features
    assert ifknn_ref.candidates_are_precision_free(f)
    for shrinkage in shrinkages:
        for k in (5, 60):
            conf = {'alg': 'ifknn', 'k': k, 'shrinkage': shrinkage, 'sim_func_params': {'sim_func_name': 'dense_cosine'}}
            model = KNNAlgorithm.build_from_conf(conf, None)
            assert isinstance(model, ItemFeatureKNN)
            sim_mtx = compute_similarity_top_k(f, model.sim_func, model.k, model.shrinkage, model.BLOCK_SIZE)   # explicit zeros kept
            model.fit(inter, f)
            pred = np.asarray(model.pred_mtx.todense() if sp.issparse(model.pred_mtx) else model.pred_mtx, dtype=np.float64)
            name = f'ifknn_{which}_s{int(shrinkage)}_k{k}'
            arrays[f'{name}/sim/indptr'], arrays[f'{name}/sim/indices'] = sim_mtx.indptr.astype(np.int64), sim_mtx.indices.astype(np.int64)
            arrays[f'{name}/sim/data'], arrays[f'{name}/pred_mtx'] = sim_mtx.data.astype(np.float64), pred
            v64, cand = ifknn_ref.values(f, shrinkage)
            n_cand = cand.sum(axis=1)
            tied = int(ifknn_ref.boundary_tied(v64, cand, k).sum())
            rows = ifknn_ref.fixture_rows(sim_mtx.indptr, sim_mtx.indices, sim_mtx.data)
            assert n_cand[ZERO_ROW] == 0 and len(rows[ZERO_ROW][0]) == 0
            if k == 60:
                assert int(n_cand.max()) < k and all(len(r[0]) == c for r, c in zip(rows, n_cand)), f'{name}: the reference pruned a row'
                assert all(i in r[0] and r[1][list(r[0]).index(i)] == 0 for i, r in enumerate(rows) if i != ZERO_ROW), f'{name}: no self 0'
            else:
                assert tied <= MAX_TIED_FRACTION * len(n_cand), f'{name}: {tied} of {len(n_cand)} rows tied at the boundary'
            meta['cases'].append({'name': name, 'features': which, 'shrinkage': shrinkage, 'k': k, 'model_name': model.name,
                                  'rows': int(len(n_cand)), 'max_candidates': int(n_cand.max()), 'rows_tied_at_boundary': tied,
                                  'min_value': float(sim_mtx.data.min()), 'max_value': float(sim_mtx.data.max())})
np.savez_compressed(os.path.join(HERE, 'g25_ifknn.npz'), **arrays)
json.dump(meta, open(os.path.join(HERE, 'g25_ifknn.json'), 'w'), indent=1)
print('g25', len(arrays), [(c['name'], c['rows_tied_at_boundary'], c['min_value'], c['max_value']) for c in meta['cases']])
