#!/usr/bin/env python3
"""G19: ACF (algorithms/sgd_alg.py:203-329, Barkan et al., CIKM 2021), generated with the REAL reference.

    PYTHONHASHSEED=0 python tests/golden/make_golden_acf.py      (build container only)

Per case: the state_dict, train-mode logits of the shared batch, every entry of get_and_reset_other_loss, the BCE and BPR losses
(train/rec_losses.py:40-83), the gradient of every parameter of rec_loss + reg_loss under each loss (train/trainer.py:205-215), eval-mode
all-pairs scores through get_*_representations + combine (eval/eval.py:205-217), the pre_tune / post_tune outputs of both sides and
post_val(0) (explanations/utils.py:223-257 with compute_cosine_sim). Only data is written: g19_acf.npz + g19_acf.json.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the import placeholders, asserts PYTHONHASHSEED=0)

import torch  # noqa: E402
from algorithms.sgd_alg import ACF  # noqa: E402
from train.rec_losses import RecBayesianPersonalizedRankingLoss, RecBinaryCrossEntropy  # noqa: E402

U, I = G.U, G.I
u, i, labels = G.batch(19)
losses = {
    'bce': RecBinaryCrossEntropy(n_items=I, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=3),
    'bpr': RecBayesianPersonalizedRankingLoss(n_items=I, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=3),
}

# (a): the default deltas; (b), (c): unequal, mutually different, non-default deltas; (d): unit weights at the smallest anchor count
CASES = [
    ('a_default', dict(embedding_dim=12, n_anchors=5, delta_exc=1e-1, delta_inc=1e-2)),
    ('b_weights', dict(embedding_dim=10, n_anchors=7, delta_exc=0.3, delta_inc=0.05)),
    ('c_weights', dict(embedding_dim=9, n_anchors=4, delta_exc=0.02, delta_inc=0.7)),
    ('d_two_anchors', dict(embedding_dim=6, n_anchors=2, delta_exc=1., delta_inc=1.)),
]

ds = G.make_dataset()
arrays = dict(G.world_arrays())
arrays['u'], arrays['i'], arrays['labels'] = G.t2n(u), G.t2n(i), G.t2n(labels)
meta = {'cases': []}
for n_case, (name, conf) in enumerate(CASES):
    torch.manual_seed(190 + n_case)
    m = ACF.build_from_conf(conf, ds)           # N(0, 1) anchors and embeddings: the reference's own initialisation is kept
    arrays.update(G.sd2n(m.state_dict(), f'{name}/sd/'))
    m.train()
    for l_name, loss_fn in losses.items():
        m.zero_grad()
        logits = m(u, i)
        rec = loss_fn.compute_loss(logits, labels)
        reg = m.get_and_reset_other_loss()
        (rec + reg['reg_loss']).backward()
        arrays[f'{name}/loss_{l_name}'] = G.t2n(rec)
        for k, v in reg.items():
            arrays[f'{name}/other_{l_name}/{k}'] = G.t2n(v)
        for p_name, p in m.named_parameters():
            arrays[f'{name}/grad_{l_name}/{p_name}'] = G.t2n(p.grad)
    arrays[f'{name}/logits'] = G.t2n(logits)
    m.eval()
    with torch.no_grad():
        all_items = torch.arange(I)
        ir = m.get_item_representations(all_items)
        arrays[f'{name}/scores_all'] = G.t2n(m.combine_user_item_representations(m.get_user_representations(u), ir))
        c_u = m.get_user_representations_pre_tune(u)
        c_i = m.get_item_representations_pre_tune(i)
        arrays[f'{name}/user_pre_tune'] = G.t2n(c_u)
        arrays[f'{name}/item_pre_tune'] = G.t2n(c_i)
        arrays[f'{name}/user_post_tune'] = G.t2n(m.get_user_representations_post_tune(c_u))
        i_post = m.get_item_representations_post_tune(c_i)
        assert len(i_post) == 3 and i_post[1] is c_i and i_post[2] is None
        arrays[f'{name}/item_post_tune'] = G.t2n(i_post[0])
    post_val = {k: float(v) for k, v in m.post_val(0).items()}
    meta['cases'].append({'name': name, 'alg': 'acf', 'conf': conf, 'keys': list(m.state_dict().keys()), 'other_keys': list(reg.keys()),
                          'model_name': m.name, 'post_val': post_val})
np.savez_compressed(os.path.join(HERE, 'g19_acf.npz'), **arrays)
json.dump(meta, open(os.path.join(HERE, 'g19_acf.json'), 'w'), indent=1)
print('g19', len(arrays), [(c['name'], c['keys']) for c in meta['cases']])
