#!/usr/bin/env python3
"""G21: UProtoMFs / IProtoMFs / UIProtoMFs (algorithms/sgd_alg.py:643-850), generated with the REAL reference.

    PYTHONHASHSEED=0 python tests/golden/make_golden_protomfs.py      (build container only)

Per case: the state_dict, train-mode logits of the shared batch, the BCE and BPR losses (train/rec_losses.py:40-83), the gradient of every
parameter under each loss (train/trainer.py:205-215; this family has no regulariser), eval-mode all-pairs scores through
get_*_representations + combine (eval/eval.py:205-217) and the scalar entries of post_val(0) (explanations/utils.py:260-300; the images
are dropped). Only data is written: g21_protomfs.npz + g21_protomfs.json.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the import placeholders, asserts PYTHONHASHSEED=0)

import torch  # noqa: E402
from algorithms.sgd_alg import IProtoMFs, UIProtoMFs, UProtoMFs  # noqa: E402
from train.rec_losses import RecBayesianPersonalizedRankingLoss, RecBinaryCrossEntropy  # noqa: E402
import explanations.utils as XU  # noqa: E402


class _Blank:
    """stands in for the plotting packages of post_val: the t-SNE picture and the two histograms are not recorded (the installed t-SNE
    refuses the reference's arguments), the scalar entries next to them are the reference's own arithmetic"""

    def __call__(self, *a, **k):
        return _Blank()

    def __getattr__(self, item):
        return _Blank()


XU.tsne_plot = XU.plt = XU.Image = XU.wandb = XU.matplotlib = _Blank()

U, I = G.U, G.I
u, i, labels = G.batch(21)
losses = {
    'bce': RecBinaryCrossEntropy(n_items=I, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=3),
    'bpr': RecBayesianPersonalizedRankingLoss(n_items=I, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=3),
}
CLASSES = {'uprotomfs': UProtoMFs, 'iprotomfs': IProtoMFs, 'uiprotomfs': UIProtoMFs}

# (a)-(c): every class once (UIProtoMFs with unequal prototype counts); (d): a UProtoMFs whose embedding row of the first user of the
# batch is all zero — F.normalize's eps clamp is what keeps it finite; (e), (f): weight tables (the item side of a UProtoMFs, the user
# side of an IProtoMFs) in which every fourth entry is exactly zero and the rest of either sign: the ReLU gate at and below its kink
CASES = [
    ('a_u', 'uprotomfs', dict(embedding_dim=12, n_prototypes=5), None),
    ('b_i', 'iprotomfs', dict(embedding_dim=12, n_prototypes=7), None),
    ('c_ui_5_7', 'uiprotomfs', dict(embedding_dim=12, u_n_prototypes=5, i_n_prototypes=7), None),
    ('d_u_zero_row', 'uprotomfs', dict(embedding_dim=12, n_prototypes=5), 'zero_row'),
    ('e_u_relu_gate', 'uprotomfs', dict(embedding_dim=10, n_prototypes=6), 'gate'),
    ('f_i_relu_gate', 'iprotomfs', dict(embedding_dim=9, n_prototypes=4), 'gate'),
]

ds = G.make_dataset()
arrays = dict(G.world_arrays())
arrays['u'], arrays['i'], arrays['labels'] = G.t2n(u), G.t2n(i), G.t2n(labels)
meta = {'cases': []}
for n_case, (name, alg, conf, special) in enumerate(CASES):
    torch.manual_seed(210 + n_case)
    m = CLASSES[alg].build_from_conf(conf, ds)
    zero_user = None
    with torch.no_grad():
        for p_name, p in m.named_parameters():
            # the initial scale (std 0.1 / dim) makes every cosine's gradient huge and the logits tiny: unit-scale values give signal
            p.copy_(torch.randn_like(p) * (0.5 if 'prototypes' in p_name or 'embed' in p_name else 0.3))
        if special == 'zero_row':
            zero_user = int(u[0])
            m.user_embed.weight[zero_user] = 0.
        if special == 'gate':
            w = (m.item_embed if alg == 'uprotomfs' else m.user_embed).weight
            w.view(-1)[::4] = 0.
    arrays.update(G.sd2n(m.state_dict(), f'{name}/sd/'))
    m.train()
    for l_name, loss_fn in losses.items():
        m.zero_grad()
        logits = m(u, i)
        rec = loss_fn.compute_loss(logits, labels)
        rec.backward()
        arrays[f'{name}/loss_{l_name}'] = G.t2n(rec)
        for p_name, p in m.named_parameters():
            arrays[f'{name}/grad_{l_name}/{p_name}'] = G.t2n(p.grad)
    arrays[f'{name}/logits'] = G.t2n(logits)
    m.eval()
    with torch.no_grad():
        ir = m.get_item_representations(torch.arange(I))
        arrays[f'{name}/scores_all'] = G.t2n(m.combine_user_item_representations(m.get_user_representations(u), ir))
    post_val = {k: float(v) for k, v in m.post_val(0).items() if isinstance(v, (float, np.floating))}
    meta['cases'].append({'name': name, 'alg': alg, 'conf': conf, 'keys': list(m.state_dict().keys()), 'special': special,
                          'zero_user': zero_user, 'model_name': m.name, 'post_val': post_val})
np.savez_compressed(os.path.join(HERE, 'g21_protomfs.npz'), **arrays)
json.dump(meta, open(os.path.join(HERE, 'g21_protomfs.json'), 'w'), indent=1)
print('g21', len(arrays), [(c['name'], c['keys'], list(c['post_val'])) for c in meta['cases']])
