"""Plain-torch CPU restatement of ECF (algorithms/sgd_alg.py:891-1138) over a flat state_dict — a test helper, not a test. Dense and
sparse-free; it computes in the dtype of the tensors it is given, so a float64 copy of the parameters serves as the truth.

    sd      {'clusters': [C, D], 'user_embed.weight': [U, D], 'item_embed.weight': [I, D]}
    conf    the build_from_conf dictionary, merged over DEFAULTS
    inter   [U, I] dense interaction matrix, tag [I, T] dense weighted tag matrix (both in the dtype of sd)

Ties at a mask boundary go to the lowest cluster index (a stable descending sort), the rule of csrc/cluster_affil.hip.
"""
import numpy as np
import torch
from torch.nn import functional as F

DEFAULTS = dict(embedding_dim=100, n_clusters=64, top_n=20, top_m=20, temp_masking=2., temp_tags=2., top_p=4, lam_cf=0.6, lam_ind=1.,
                lam_ts=1.)


def cosine_sim(x, y):
    """sgd_alg.py:62-73."""
    return torch.clamp(F.normalize(x) @ F.normalize(y).T, min=-1., max=1.)


def top_mask(t, top):
    """1 at the ``top`` largest entries of every row; equal values: the lowest index first."""
    order = torch.sort(t.detach(), dim=-1, descending=True, stable=True).indices[..., :top]
    return torch.zeros_like(t).scatter_(-1, order, 1.)


def affiliation(t, top, temp):
    """sgd_alg.py:994-1007 / 1024-1037 behind the logits: sigmoid(t) * (p + (m - p).detach())."""
    m = top_mask(t, top)
    p = torch.softmax(t / temp, dim=-1)
    return torch.sigmoid(t) * (p + (m - p).detach())


def tag_matrix(n_items, item_idx, tag_idx, n_tags):
    """data/dataset.py:469-483, dense float64 [n_items, n_tags]."""
    m = np.zeros((n_items, n_tags))
    np.add.at(m, (np.asarray(item_idx), np.asarray(tag_idx)), 1.)
    return m * np.log(n_items / (m.sum(axis=0) + 1e-6))[None, :]


def items(sd, conf):
    """-> (x_tildes, xs), [I, C] each."""
    p = {**DEFAULTS, **conf}
    x_tildes = cosine_sim(sd['item_embed.weight'], sd['clusters'])
    return x_tildes, affiliation(x_tildes, p['top_m'], p['temp_masking'])


def users(sd, conf, inter, u, x_tildes):
    """-> (a_tilde, a), [B, C] each."""
    p = {**DEFAULTS, **conf}
    a_tilde = inter[torch.as_tensor(u).long()] @ x_tildes
    return a_tilde, affiliation(a_tilde, p['top_n'], p['temp_masking'])


def combine(a, x):
    """sgd_alg.py:1039-1045."""
    return (a.unsqueeze(-2) * x).sum(dim=-1)


def forward(sd, conf, inter, tag, u, i):
    """Train-mode forward + get_and_reset_other_loss: (logits [B, N], loss dictionary)."""
    p = {**DEFAULTS, **conf}
    u, i = torch.as_tensor(u).long(), torch.as_tensor(i).long()
    x_tildes, xs = items(sd, conf)
    _, a = users(sd, conf, inter, u, x_tildes)
    dots = combine(a, xs[i])
    log_b_c = F.log_softmax((xs.T @ tag) / p['temp_tags'], dim=-1)
    ts = (-log_b_c.topk(p['top_p'], dim=-1).values).sum()
    ind = torch.diag(-F.log_softmax(cosine_sim(sd['clusters'], sd['clusters']), dim=-1)).sum()
    logits = (sd['user_embed.weight'][u].unsqueeze(-2) * sd['item_embed.weight'][i]).sum(dim=-1)
    diff = (logits[:, :1] - logits[:, 1:]).flatten()
    cf = F.binary_cross_entropy_with_logits(diff, torch.ones_like(diff))
    cf_loss, ind_loss, ts_loss = p['lam_cf'] * cf, p['lam_ind'] * ind, p['lam_ts'] * ts
    return dots, {'reg_loss': ts_loss + ind_loss + cf_loss, 'cf_loss': cf_loss, 'ind_loss': ind_loss, 'ts_loss': ts_loss}


def scores_all(sd, conf, inter, u):
    """eval/eval.py:205-217: the users u against every item."""
    x_tildes, xs = items(sd, conf)
    return users(sd, conf, inter, u, x_tildes)[1] @ xs.T


def pre_tune(sd, conf, inter, u):
    """-> ((xs, item table), (a, user rows)): sgd_alg.py:1047-1066, 1073-1093; post_tune is the identity."""
    x_tildes, xs = items(sd, conf)
    return (xs, sd['item_embed.weight']), (users(sd, conf, inter, u, x_tildes)[1], sd['user_embed.weight'][torch.as_tensor(u).long()])


def post_tune(repr_):
    return repr_


def rec_loss(kind, logits, labels):
    """train/rec_losses.py:56 (bce) and :73-83 (bpr), aggregator 'mean', with torch's own BCE-with-logits as the reference has it: its
    gradient at a logit of exactly 0 is sigmoid(0) - y. ECF's scores ARE exactly 0 wherever the user's and the item's masks are disjoint,
    and oracle/losses_ref.py composes the loss from clamp and abs, whose autograd subgradients at 0 add up to 1 - y: right in value, not
    in gradient at that one point, so the ECF tests do not use it."""
    if kind == 'bce':
        return F.binary_cross_entropy_with_logits(logits.flatten(), labels.flatten())
    diff = logits[:, :1] - logits[:, 1:]
    target = torch.repeat_interleave(labels[:, 0], diff.shape[1])
    return F.binary_cross_entropy_with_logits(diff.flatten(), target.flatten())


def gap(t, top):
    """per row: the distance between the top-th and the next value (inf when top == number of columns)"""
    s = torch.sort(t, dim=-1, descending=True).values
    if top >= t.shape[-1]:
        return torch.full(t.shape[:-1], float('inf'), dtype=t.dtype)
    return s[..., top - 1] - s[..., top]
