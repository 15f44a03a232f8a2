#!/usr/bin/env python3
"""G27: PopularItems (algorithms/naive_algs.py:35-60) and the popularity formula (data/dataset.py:357-359), generated with the REAL reference.

    PYTHONHASHSEED=0 python tests/golden/make_golden_naive.py      (build container only)

A 12-user x 9-item 0/1 matrix with tied column counts and one empty column. Recorded: the matrix; ``pop``, the value of
``TrainRecDataset._get_pop_distribution`` on it (float64); arbitrary ``u_idxs`` [7] / ``i_idxs`` [7, 5], repeats included; and
``PopularItems(pop).predict(u_idxs, i_idxs)`` (float64). ``RandomItems`` draws from the CPU's global generator: nothing of it is a fixture.
Only data is written: g27_naive.npz + g27_naive.json.
"""
import json
import os
import sys
import warnings
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402,F401  (installs the import placeholders, asserts PYTHONHASHSEED=0)

import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402
from algorithms.naive_algs import PopularItems  # noqa: E402
from data.dataset import TrainRecDataset  # noqa: E402

if __name__ == '__main__':
    rng = np.random.default_rng(27)
    counts = [5, 3, 0, 5, 1, 8, 3, 3, 12]                    # per item: ties at 5 and at 3, an item nobody holds, an item everybody holds
    dense = np.zeros((12, 9))
    for i, c in enumerate(counts):
        dense[rng.choice(12, size=c, replace=False), i] = 1
    inter = sp.csr_matrix(dense)
    pop = TrainRecDataset._get_pop_distribution(SimpleNamespace(user_sampling_matrix=inter))
    assert pop.dtype == np.float64 and pop.shape == (9,) and np.array_equal(pop * inter.nnz, np.asarray(counts, dtype=np.float64))
    model = PopularItems.build_from_conf({}, SimpleNamespace(pop_distribution=pop))
    u_idxs = torch.from_numpy(rng.integers(0, 12, size=7))
    i_idxs = torch.from_numpy(rng.integers(0, 9, size=(7, 5)))
    i_idxs[0] = torch.tensor([2, 2, 8, 0, 3])                # the empty item twice, the two tied at 5
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        pred = model.predict(u_idxs, i_idxs)
    assert pred.dtype == torch.float64 and tuple(pred.shape) == (7, 5)
    np.savez_compressed(os.path.join(HERE, 'g27_naive.npz'), inter=dense, pop=pop, u_idxs=u_idxs.numpy(), i_idxs=i_idxs.numpy(),
                        predict=pred.numpy())
    meta = {'model_name': model.name, 'users': 12, 'items': 9, 'counts': counts, 'nnz': int(inter.nnz), 'torch': torch.__version__,
            'numpy': np.__version__}
    json.dump(meta, open(os.path.join(HERE, 'g27_naive.json'), 'w'), indent=1)
    print('g27', meta)
