#!/usr/bin/env python3
"""G20: ECF (algorithms/sgd_alg.py:891-1138, Du et al., WWW 2023), generated with the REAL reference.

    PYTHONHASHSEED=0 python tests/golden/make_golden_ecf.py      (build container only)

Per case: the state_dict (with the reference's ``interaction_matrix`` entry: the matrix is handed over as float32), train-mode logits of the
shared batch, every entry of get_and_reset_other_loss, the BCE and BPR losses (train/rec_losses.py:40-83), the gradient of every trainable
parameter of rec_loss + reg_loss under each loss (train/trainer.py:205-215), eval-mode all-pairs scores through get_*_representations +
combine (eval/eval.py:205-217) and the pre_tune / post_tune outputs of both sides. The tag matrix comes from the reference's own
ECFTrainRecDataset._prepare_tag_data (data/dataset.py:469-483) run on two temporary CSV files. Only data is written: g20_ecf.npz +
g20_ecf.json.

The reference's ECF.__init__ reads ``scipy_matrix.A``, which current scipy no longer has: it is handed a small object with an ``.A`` array.

torch.topk leaves the order of ties open, so every case's seed is advanced until, in float64, no mask boundary is closer than 1e-4 (item
and recorded user logits) and no top_p boundary of the tag loss closer than 1e-5.
"""
import json
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402  (installs the import placeholders, asserts PYTHONHASHSEED=0)

import pandas as pd  # noqa: E402
import torch  # noqa: E402
from algorithms.sgd_alg import ECF  # noqa: E402
from data.dataset import ECFTrainRecDataset  # noqa: E402
from train.rec_losses import RecBayesianPersonalizedRankingLoss, RecBinaryCrossEntropy  # noqa: E402

import ecf_ref  # noqa: E402

U, I, T = G.U, G.I, 9
u, i, labels = G.batch(20)
losses = {
    'bce': RecBinaryCrossEntropy(n_items=I, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=3),
    'bpr': RecBayesianPersonalizedRankingLoss(n_items=I, aggregator='mean', train_neg_strategy='uniform_recbole', neg_train=3),
}

# (a): a small dimension, default temperatures and weights; (b): unequal non-default weights and temperatures (n_clusters % 4 == 0);
# (c): top_m = top_n = n_clusters, the all-ones mask; (d): two clusters, one of them kept
CASES = [
    ('a_default', dict(embedding_dim=8, n_clusters=6, top_n=2, top_m=2)),
    ('b_weights', dict(embedding_dim=10, n_clusters=8, top_n=3, top_m=4, temp_masking=1.5, temp_tags=0.7, top_p=3, lam_cf=0.3, lam_ind=0.45,
                       lam_ts=0.2)),
    ('c_all_ones', dict(embedding_dim=7, n_clusters=5, top_n=5, top_m=5)),
    ('d_two_clusters', dict(embedding_dim=6, n_clusters=2, top_n=1, top_m=1, top_p=2)),
]


class _HasA:
    """what ECF.__init__ reads of a scipy matrix (sgd_alg.py:905-906)"""

    def __init__(self, m, dtype):
        self.A = np.asarray(m.toarray(), dtype=dtype)


def tag_world():
    """item-tag pairs: 1 to 3 tags per item, every tag used, no two tags with the same item set"""
    rng = np.random.default_rng(20)
    item_idx, tag_idx = [], []
    for item in range(I):
        for t in rng.choice(T, size=rng.integers(1, 4), replace=False):
            item_idx.append(item)
            tag_idx.append(int(t))
    return np.asarray(item_idx, dtype=np.int64), np.asarray(tag_idx, dtype=np.int64)


item_idx, tag_idx = tag_world()
with tempfile.TemporaryDirectory() as tmp:
    pd.DataFrame({'tag_idx': np.arange(T), 'tag': [f't{k}' for k in range(T)]}).to_csv(os.path.join(tmp, 'tag_idxs.csv'), index=False)
    pd.DataFrame({'item_idx': item_idx, 'tag_idx': tag_idx}).to_csv(os.path.join(tmp, 'item_tag_idxs.csv'), index=False)
    holder = SimpleNamespace(data_path=tmp, n_items=I, tag_matrix=None)
    ECFTrainRecDataset._prepare_tag_data(holder)
tag_matrix = holder.tag_matrix.tocsr()
tag_dense = tag_matrix.toarray()
assert tag_dense.shape == (I, T) and bool(((tag_dense != 0).sum(axis=0) >= 1).all()), 'every tag has at least one item'
assert len({tuple(col) for col in tag_dense.T}) == T, 'no two tag columns are equal'

ds = G.make_dataset()
inter = ds.user_sampling_matrix_train
assert bool((np.asarray(inter[G.t2n(u)].sum(axis=1)).ravel() >= 1).all()), 'every batch user has at least one interaction'
inter64, tag64 = torch.from_numpy(inter.toarray().astype(np.float64)), torch.from_numpy(tag_dense.astype(np.float32).astype(np.float64))


def conditions_hold(sd, conf):
    p = {**ecf_ref.DEFAULTS, **conf}
    sd64 = {k: v.detach().double() for k, v in sd.items() if k != 'interaction_matrix'}
    x_tildes, xs = ecf_ref.items(sd64, conf)
    a_tilde, _ = ecf_ref.users(sd64, conf, inter64, u, x_tildes)
    log_b_c = torch.log_softmax((xs.T @ tag64) / p['temp_tags'], dim=-1)
    gaps = (float(ecf_ref.gap(x_tildes, p['top_m']).min()), float(ecf_ref.gap(a_tilde, p['top_n']).min()),
            float(ecf_ref.gap(log_b_c, p['top_p']).min()))
    return gaps[0] >= 1e-4 and gaps[1] >= 1e-4 and gaps[2] >= 1e-5, gaps


arrays = dict(G.world_arrays())
arrays['u'], arrays['i'], arrays['labels'] = G.t2n(u), G.t2n(i), G.t2n(labels)
arrays['tags/item_idx'], arrays['tags/tag_idx'], arrays['tags/n_tags'] = item_idx, tag_idx, np.array(T)
arrays['tags/matrix'] = tag_dense                                                  # float64 [I, T], the reference's weighted matrix
meta = {'cases': []}
for n_case, (name, conf) in enumerate(CASES):
    seed = 200 + 100 * n_case
    while True:
        torch.manual_seed(seed)
        data = SimpleNamespace(n_users=U, n_items=I, tag_matrix=_HasA(tag_matrix, np.float64), sampling_matrix=_HasA(inter, np.float32))
        m = ECF.build_from_conf(conf, data)
        ok, gaps = conditions_hold(m.state_dict(), conf)
        if ok:
            break
        seed += 1
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
            if p.requires_grad:
                arrays[f'{name}/grad_{l_name}/{p_name}'] = G.t2n(p.grad)
    arrays[f'{name}/logits'] = G.t2n(logits)
    m.eval()
    with torch.no_grad():
        ir = m.get_item_representations(torch.arange(I))
        arrays[f'{name}/scores_all'] = G.t2n(m.combine_user_item_representations(m.get_user_representations(u), ir))
        xs, table = m.get_item_representations_pre_tune(i)
        a, rows = m.get_user_representations_pre_tune(u)
        arrays[f'{name}/item_pre_tune/0'], arrays[f'{name}/item_pre_tune/1'] = G.t2n(xs), G.t2n(table)
        arrays[f'{name}/user_pre_tune/0'], arrays[f'{name}/user_pre_tune/1'] = G.t2n(a), G.t2n(rows)
        i_post, u_post = m.get_item_representations_post_tune((xs, table)), m.get_user_representations_post_tune((a, rows))
        assert i_post[0] is xs and i_post[1] is table and u_post[0] is a and u_post[1] is rows      # post_tune is the identity
    meta['cases'].append({'name': name, 'alg': 'ecf', 'conf': conf, 'seed': seed, 'keys': list(m.state_dict().keys()),
                          'other_keys': list(reg.keys()), 'model_name': m.name, 'min_gaps_item_user_tag': [g if np.isfinite(g) else None for g in gaps]})
np.savez_compressed(os.path.join(HERE, 'g20_ecf.npz'), **arrays)
json.dump(meta, open(os.path.join(HERE, 'g20_ecf.json'), 'w'), indent=1)
print('g20', len(arrays), [(c['name'], c['seed'], c['keys'], c['min_gaps_item_user_tag']) for c in meta['cases']])
