#!/usr/bin/env python3
"""G17: DeepMatrixFactorization (algorithms/sgd_alg.py:1141-1276), generated with the REAL reference.

    PYTHONHASHSEED=0 python tests/golden/make_golden_dmf.py      (build container only)

Per case: the state_dict, train-mode logits of the shared batch, the BCE and BPR losses (train/rec_losses.py:40-83), the gradient of
every parameter under each loss, eval-mode all-pairs scores through get_*_representations + combine (eval/eval.py:205-217), and the
fraction of floored logits (``sim[sim < mu] = mu``, sgd_alg.py:1241). Only data is written: g17_deepmf.npz + g17_deepmf.json.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the import placeholders, asserts PYTHONHASHSEED=0)

import torch  # noqa: E402
from algorithms.sgd_alg import DeepMatrixFactorization  # noqa: E402
from data.dataset import InteractionRecDataset  # noqa: E402
from train.rec_losses import RecBayesianPersonalizedRankingLoss, RecBinaryCrossEntropy  # noqa: E402

U, I = G.U, G.I
u, i, labels = G.batch(17)
losses = {
    'bce': RecBinaryCrossEntropy(n_items=I, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=3),
    'bpr': RecBayesianPersonalizedRankingLoss(n_items=I, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=3),
}

# the shared world with the dataset methods DeepMF calls (data/dataset.py:260-273, 306-319)
ds = G.make_dataset()
ds._get_numpy_array = InteractionRecDataset._get_numpy_array
ds.get_user_interaction_vectors = lambda idx: InteractionRecDataset._get_interaction_vectors(ds, 'user', idx)
ds.get_item_interaction_vectors = lambda idx: InteractionRecDataset._get_interaction_vectors(ds, 'item', idx)

# (a) has mu = -1: a cosine is never below it, so the case runs the scorer with the floor idle (at the default mu = 1e-6 about half the
# cosines of a randomly initialised model are floored: (b), (c) and (e) cover that); (d) raises mu so that the floor bites on positive
# cosines too
CASES = [
    ('a_nomid', dict(u_mid_layers=[], i_mid_layers=[], final_dimension=8, mu=-1.0)),
    ('b_mid_outact', dict(u_mid_layers=[12], i_mid_layers=[9, 7], final_dimension=6, use_output_activation_fn=True)),
    ('c_norm_inter', dict(u_mid_layers=[10], i_mid_layers=[10], final_dimension=8, normalize_interactions=True)),
    ('d_norm_repr_floor', dict(u_mid_layers=[12], i_mid_layers=[12], final_dimension=8, normalize_representations=True, mu=0.05)),
    ('e_odd', dict(u_mid_layers=11, i_mid_layers=[13], final_dimension=5)),
    # no mid layers at the reference's default mu: layer 0 is the output layer and the floor is active
    ('f_nomid_default_mu', dict(u_mid_layers=[], i_mid_layers=[], final_dimension=8)),
]

arrays = dict(G.world_arrays())
arrays['u'], arrays['i'], arrays['labels'] = G.t2n(u), G.t2n(i), G.t2n(labels)
meta = {'cases': []}
for n_case, (name, kw) in enumerate(CASES):
    torch.manual_seed(170 + n_case)
    m = DeepMatrixFactorization(ds, **kw)
    with torch.no_grad():
        for p_name, p in m.named_parameters():
            if 'bias' in p_name:                      # biases initialise to 0: give them signal
                p.copy_(torch.randn_like(p) * 0.1)
    arrays.update(G.sd2n(m.state_dict(), f'{name}/sd/'))
    m.train()
    for l_name, loss_fn in losses.items():
        m.zero_grad()
        logits = m(u, i)
        loss = loss_fn.compute_loss(logits, labels)
        loss.backward()
        arrays[f'{name}/loss_{l_name}'] = G.t2n(loss)
        for p_name, p in m.named_parameters():
            arrays[f'{name}/grad_{l_name}/{p_name}'] = G.t2n(p.grad)
    arrays[f'{name}/logits'] = G.t2n(logits)
    floored = float((logits.detach() == m.mu).double().mean())
    m.eval()
    with torch.no_grad():
        ir = m.get_item_representations(torch.arange(I))
        arrays[f'{name}/scores_all'] = G.t2n(m.combine_user_item_representations(m.get_user_representations(u), ir))
    meta['cases'].append({'name': name, 'kwargs': kw, 'keys': list(m.state_dict().keys()), 'floored_fraction': floored})
np.savez_compressed(os.path.join(HERE, 'g17_deepmf.npz'), **arrays)
json.dump(meta, open(os.path.join(HERE, 'g17_deepmf.json'), 'w'), indent=1)
print('g17', len(arrays), [(c['name'], c['floored_fraction']) for c in meta['cases']])
