"""Plain-torch CPU restatement of ACF (algorithms/sgd_alg.py:203-329) over a flat state_dict — a test helper, not a test. It computes in
the dtype of the tensors it is given, so a float64 copy of the parameters serves as the truth.

    sd      {'anchors': [K, D], 'user_embed.weight': [U, D], 'item_embed.weight': [I, D]}
    conf    the build_from_conf dictionary (delta_exc, delta_inc)
"""
import math

import torch
from torch.nn import functional as F

MAX_ENTITIES = 10000


def entropy_from_softmax(p, p_unnorm):
    """sgd_alg.py:76-85."""
    return (-(p * (p_unnorm - torch.logsumexp(p_unnorm, dim=-1, keepdim=True)))).sum(-1)


def mix(e, anchors):
    """sgd_alg.py:261-276 on gathered rows: (r, c, logits)."""
    s = e @ anchors.T
    c = torch.softmax(s, dim=-1)
    return c @ anchors, c, s


def losses(c, s):
    """sgd_alg.py:246-254 -> (exc, inc), unweighted. A column of c that is 0 everywhere gives inc = NaN (0 log 0), as in the reference."""
    K = c.shape[-1]
    exc = entropy_from_softmax(c, s).mean()
    q = c.reshape(-1, K).sum(dim=0) / c.sum()
    inc = math.log(K) - (-q * torch.log(q)).sum()
    return exc, inc


def q_of(c):
    return c.reshape(-1, c.shape[-1]).sum(dim=0) / c.sum()


def side(sd, which, idx):
    idx = torch.as_tensor(idx).long()
    return mix(sd[f'{which}_embed.weight'][idx], sd['anchors'])


def combine(u_anc, i_anc):
    """sgd_alg.py:278-283."""
    return (u_anc.unsqueeze(-2) * i_anc).sum(dim=-1)


def forward(sd, conf, u, i):
    """Train-mode forward + get_and_reset_other_loss: (logits [B, N], loss dictionary)."""
    u_anc, _, _ = side(sd, 'user', u)
    i_anc, c_i, s_i = side(sd, 'item', i)
    exc, inc = losses(c_i, s_i)
    exc_loss, inc_loss = conf['delta_exc'] * exc, conf['delta_inc'] * inc
    return combine(u_anc, i_anc), {'reg_loss': exc_loss + inc_loss, 'exc_loss': exc_loss, 'inc_loss': inc_loss}


def scores_all(sd, u, n_items):
    """eval/eval.py:205-217: the users u against every item."""
    return combine(side(sd, 'user', u)[0], side(sd, 'item', torch.arange(n_items))[0])


def pre_tune(sd, which, idx):
    return side(sd, which, idx)[1]


def post_tune(sd, c):
    return c @ sd['anchors']


def cosine_sim(x, y):
    """sgd_alg.py:62-73."""
    return torch.clamp(F.normalize(x) @ F.normalize(y).T, min=-1., max=1.)


def post_val(sd):
    """explanations/utils.py:223-257 with sim_func = compute_cosine_sim on the anchors and the item table, the full (K + n)^2 matrix."""
    with torch.no_grad():
        anchors, entities = sd['anchors'], sd['item_embed.weight']
        n = len(anchors)
        if len(entities) >= MAX_ENTITIES:
            entities = entities[torch.randperm(len(entities))[:MAX_ENTITIES]]
        both = torch.cat([anchors, entities])
        sim_mtx = cosine_sim(both, both)
        e2p = sim_mtx[n:, :n]
        return {'avg_pairwise_proto_sim': ((torch.tril(sim_mtx[:n, :n], diagonal=-1).sum() * 2) / (n * (n - 1))).item(),
                'entity_to_proto_mean': e2p.mean(dim=-1).mean().item(), 'entity_to_proto_max': e2p.max(dim=-1).values.mean().item(),
                'entity_to_proto_min': e2p.min(dim=-1).values.mean().item()}


def nan_case(dtype=torch.float32, logit=200.):
    """Four rows against two anchors with logits (logit, 0): at logit = 200 exp(-200) underflows in fp32 (c = [1, 0] in every row, so
    q = [1, 0] and inc = NaN); float64 needs logit >= 746 for the same. -> (table [4, 2], anchors [2, 2])"""
    table = torch.tensor([[logit, 0.]] * 4, dtype=dtype)
    anchors = torch.tensor([[1., 0.], [0., 1.]], dtype=dtype)
    return table, anchors
