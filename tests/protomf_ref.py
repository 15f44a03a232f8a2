"""Plain-torch CPU restatement of UProtoMF / IProtoMF / UIProtoMF (algorithms/sgd_alg.py:332-640) over a flat state_dict — a test helper,
not a test. It computes in the dtype of the state_dict it is given, so a float64 copy of the parameters serves as the truth.

    alg     'uprotomf' | 'iprotomf' | 'uiprotomf'
    sd      {'prototypes': ..., 'user_embed.weight': ..., 'item_embed.weight': ...}                  (uprotomf, iprotomf)
            {'uprotomf.prototypes', 'uprotomf.user_embed.weight', 'iprotomf.prototypes', 'iprotomf.item_embed.weight',
             'u_to_i_proj.weight', 'i_to_u_proj.weight'}                                             (uiprotomf)
    conf    the build_from_conf dictionary (the regulariser weights)
"""
import torch
from torch.nn import functional as F

MAX_ENTITIES = 10000


def shifted_cosine_sim(x, y):
    """sgd_alg.py:48-59."""
    return torch.clamp(1 + F.normalize(x) @ F.normalize(y).T, min=0., max=2.)


def reg_losses(sim_mtx):
    """sgd_alg.py:394-399 -> (proto term, batch term), unweighted."""
    dis_mtx = 2 - sim_mtx.reshape(-1, sim_mtx.shape[-1])
    return dis_mtx.min(dim=0).values.mean(), dis_mtx.min(dim=1).values.mean()


def sim_side(table, idx, prototypes):
    """sgd_alg.py:381-384 / 486-491: [*idx.shape, P]."""
    idx = torch.as_tensor(idx).long()
    e = table[idx.reshape(-1)]
    return shifted_cosine_sim(e, prototypes).reshape(list(idx.shape) + [prototypes.shape[0]])


def _other(proto, batch, w_proto, w_batch):
    proto_loss, batch_loss = w_proto * proto, w_batch * batch
    return {'reg_loss': proto_loss + batch_loss, 'proto_loss': proto_loss, 'batch_loss': batch_loss}


def representations(alg, sd, side, idx):
    """get_user_representations / get_item_representations."""
    idx = torch.as_tensor(idx).long()
    if alg == 'uiprotomf':
        if side == 'user':
            table = sd['uprotomf.user_embed.weight']
            return sim_side(table, idx, sd['uprotomf.prototypes']), table[idx] @ sd['u_to_i_proj.weight'].T
        table = sd['iprotomf.item_embed.weight']
        return sim_side(table, idx, sd['iprotomf.prototypes']), table[idx] @ sd['i_to_u_proj.weight'].T
    if (alg, side) in (('uprotomf', 'user'), ('iprotomf', 'item')):
        return sim_side(sd[f'{side}_embed.weight'], idx, sd['prototypes'])
    return sd[f'{side}_embed.weight'][idx]


def combine(alg, u_repr, i_repr):
    """combine_user_item_representations (sgd_alg.py:389-392, 585-593)."""
    if alg == 'uiprotomf':
        (u_sim, u_proj), (i_sim, i_proj) = u_repr, i_repr
        return (u_sim.unsqueeze(-2) * i_proj).sum(dim=-1) + (u_proj.unsqueeze(-2) * i_sim).sum(dim=-1)
    return (u_repr.unsqueeze(-2) * i_repr).sum(dim=-1)


def forward(alg, sd, conf, u, i):
    """Train-mode forward + get_and_reset_other_loss: (logits [B, N], loss dictionary)."""
    u_repr, i_repr = representations(alg, sd, 'user', u), representations(alg, sd, 'item', i)
    logits = combine(alg, u_repr, i_repr)
    if alg == 'uiprotomf':
        u_reg = _other(*reg_losses(u_repr[0]), conf['u_sim_proto_weight'], conf['u_sim_batch_weight'])
        i_reg = _other(*reg_losses(i_repr[0]), conf['i_sim_proto_weight'], conf['i_sim_batch_weight'])
        u_reg = {'user_' + k: v for k, v in u_reg.items()}
        i_reg = {'item_' + k: v for k, v in i_reg.items()}
        return logits, {'reg_loss': u_reg.pop('user_reg_loss') + i_reg.pop('item_reg_loss'), **u_reg, **i_reg}
    sim = u_repr if alg == 'uprotomf' else i_repr
    return logits, _other(*reg_losses(sim), conf['sim_proto_weight'], conf['sim_batch_weight'])


def scores_all(alg, sd, u, n_items):
    """eval/eval.py:205-217: the users u against every item."""
    return combine(alg, representations(alg, sd, 'user', u), representations(alg, sd, 'item', torch.arange(n_items)))


def _post_val_light(prototypes, entities):
    """explanations/utils.py:223-257 with sim_func = compute_shifted_cosine_sim, the full (P + n)^2 matrix as in the reference."""
    n = len(prototypes)
    if len(entities) >= MAX_ENTITIES:
        entities = entities[torch.randperm(len(entities))[:MAX_ENTITIES]]
    both = torch.cat([prototypes, entities])
    sim_mtx = shifted_cosine_sim(both, both)
    e2p = sim_mtx[n:, :n]
    return {'avg_pairwise_proto_sim': ((torch.tril(sim_mtx[:n, :n], diagonal=-1).sum() * 2) / (n * (n - 1))).item(),
            'entity_to_proto_mean': e2p.mean(dim=-1).mean().item(), 'entity_to_proto_max': e2p.max(dim=-1).values.mean().item(),
            'entity_to_proto_min': e2p.min(dim=-1).values.mean().item()}


def post_val(alg, sd):
    with torch.no_grad():
        if alg == 'uprotomf':
            return _post_val_light(sd['prototypes'], sd['user_embed.weight'])
        if alg == 'iprotomf':
            return _post_val_light(sd['prototypes'], sd['item_embed.weight'])
        u = _post_val_light(sd['uprotomf.prototypes'], sd['uprotomf.user_embed.weight'])
        i = _post_val_light(sd['iprotomf.prototypes'], sd['iprotomf.item_embed.weight'])
        return {**{'user_' + k: v for k, v in u.items()}, **{'item_' + k: v for k, v in i.items()}}
