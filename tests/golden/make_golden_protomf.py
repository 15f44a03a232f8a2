#!/usr/bin/env python3
"""G18: UProtoMF / IProtoMF / UIProtoMF (algorithms/sgd_alg.py:332-640), generated with the REAL reference.

    PYTHONHASHSEED=0 python tests/golden/make_golden_protomf.py      (build container only)

Per case: the state_dict, train-mode logits of the shared batch, every entry of get_and_reset_other_loss, the BCE and BPR losses
(train/rec_losses.py:40-83), the gradient of every parameter of rec_loss + reg_loss under each loss (train/trainer.py:205-215), eval-mode
all-pairs scores through get_*_representations + combine (eval/eval.py:205-217) and post_val(0) (explanations/utils.py:223-257).
Only data is written: g18_protomf.npz + g18_protomf.json.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the import placeholders, asserts PYTHONHASHSEED=0)

import torch  # noqa: E402
from algorithms.sgd_alg import IProtoMF, UIProtoMF, UProtoMF  # noqa: E402
from train.rec_losses import RecBayesianPersonalizedRankingLoss, RecBinaryCrossEntropy  # noqa: E402

U, I = G.U, G.I
u, i, labels = G.batch(18)
losses = {
    'bce': RecBinaryCrossEntropy(n_items=I, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=3),
    'bpr': RecBayesianPersonalizedRankingLoss(n_items=I, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=3),
}
CLASSES = {'uprotomf': UProtoMF, 'iprotomf': IProtoMF, 'uiprotomf': UIProtoMF}

# (a)-(c): every class at unit weights (UIProtoMF with unequal prototype counts); (d)-(f): non-default, mutually different weights;
# (g): a UProtoMF whose embedding row of the first user of the batch is all zero — F.normalize's eps clamp is what keeps it finite
CASES = [
    ('a_u', 'uprotomf', dict(embedding_dim=12, n_prototypes=5, sim_proto_weight=1., sim_batch_weight=1.), None),
    ('b_i', 'iprotomf', dict(embedding_dim=12, n_prototypes=7, sim_proto_weight=1., sim_batch_weight=1.), None),
    ('c_ui_5_7', 'uiprotomf', dict(embedding_dim=12, u_n_prototypes=5, i_n_prototypes=7, u_sim_proto_weight=1., u_sim_batch_weight=1.,
                                  i_sim_proto_weight=1., i_sim_batch_weight=1.), None),
    ('d_u_weights', 'uprotomf', dict(embedding_dim=10, n_prototypes=6, sim_proto_weight=0.3, sim_batch_weight=0.05), None),
    ('e_i_weights', 'iprotomf', dict(embedding_dim=9, n_prototypes=4, sim_proto_weight=0.02, sim_batch_weight=0.7), None),
    ('f_ui_weights', 'uiprotomf', dict(embedding_dim=11, u_n_prototypes=7, i_n_prototypes=5, u_sim_proto_weight=0.4, u_sim_batch_weight=0.06,
                                      i_sim_proto_weight=0.08, i_sim_batch_weight=0.9), None),
    ('g_u_zero_row', 'uprotomf', dict(embedding_dim=12, n_prototypes=5, sim_proto_weight=0.5, sim_batch_weight=0.25), int(u[0])),
]

ds = G.make_dataset()
arrays = dict(G.world_arrays())
arrays['u'], arrays['i'], arrays['labels'] = G.t2n(u), G.t2n(i), G.t2n(labels)
meta = {'cases': []}
for n_case, (name, alg, conf, zero_user) in enumerate(CASES):
    torch.manual_seed(180 + n_case)
    m = CLASSES[alg].build_from_conf(conf, ds)
    with torch.no_grad():
        for p_name, p in m.named_parameters():
            # the initial scale (std 0.1 / dim) makes every cosine's gradient huge and the logits tiny: unit-scale values give signal
            p.copy_(torch.randn_like(p) * (0.5 if 'prototypes' in p_name or 'embed' in p_name else 0.3))
        if zero_user is not None:
            m.user_embed.weight[zero_user] = 0.
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
        ir = m.get_item_representations(torch.arange(I))
        arrays[f'{name}/scores_all'] = G.t2n(m.combine_user_item_representations(m.get_user_representations(u), ir))
    post_val = {k: float(v) for k, v in m.post_val(0).items()}
    meta['cases'].append({'name': name, 'alg': alg, 'conf': conf, 'keys': list(m.state_dict().keys()), 'other_keys': list(reg.keys()),
                          'zero_user': zero_user, 'model_name': m.name, 'post_val': post_val})
np.savez_compressed(os.path.join(HERE, 'g18_protomf.npz'), **arrays)
json.dump(meta, open(os.path.join(HERE, 'g18_protomf.json'), 'w'), indent=1)
print('g18', len(arrays), [(c['name'], c['keys']) for c in meta['cases']])
