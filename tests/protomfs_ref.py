"""Plain-torch CPU restatement of UProtoMFs / IProtoMFs / UIProtoMFs (algorithms/sgd_alg.py:643-850) over a flat state_dict — a test
helper, not a test. It computes in the dtype of the state_dict it is given, so a float64 copy of the parameters serves as the truth.

    alg     'uprotomfs' | 'iprotomfs' | 'uiprotomfs'
    sd      {'prototypes': ..., 'user_embed.weight': ..., 'item_embed.weight': ...}                  (uprotomfs, iprotomfs)
            {'uprotomfs.prototypes', 'uprotomfs.user_embed.weight', 'iprotomfs.prototypes', 'iprotomfs.item_embed.weight',
             'u_to_i_proj.weight', 'i_to_u_proj.weight'}                                             (uiprotomfs)
"""
import torch
from torch.nn import functional as F

MAX_ENTITIES = 10000


def cosine_sim(x, y):
    """sgd_alg.py:62-73."""
    return torch.clamp(F.normalize(x) @ F.normalize(y).T, min=-1., max=1.)


def cos_side(table, idx, prototypes):
    """sgd_alg.py:677-678 / 742-746: [*idx.shape, P]."""
    idx = torch.as_tensor(idx).long()
    return cosine_sim(table[idx.reshape(-1)], prototypes).reshape(list(idx.shape) + [prototypes.shape[0]])


def score(e, prototypes, w):
    """The fused op's expression: e [R, D], w [R, fan, P] -> sum_p clamp(cos(e, P_p), -1, 1) relu(w) [R, fan]."""
    return (cosine_sim(e, prototypes).unsqueeze(-2) * torch.relu(w)).sum(dim=-1)


def representations(alg, sd, side, idx):
    """get_user_representations / get_item_representations."""
    idx = torch.as_tensor(idx).long()
    if alg == 'uiprotomfs':
        if side == 'user':
            table = sd['uprotomfs.user_embed.weight']
            return cos_side(table, idx, sd['uprotomfs.prototypes']), torch.relu(table[idx] @ sd['u_to_i_proj.weight'].T)
        table = sd['iprotomfs.item_embed.weight']
        return cos_side(table, idx, sd['iprotomfs.prototypes']), torch.relu(table[idx] @ sd['i_to_u_proj.weight'].T)
    if (alg, side) in (('uprotomfs', 'user'), ('iprotomfs', 'item')):
        return cos_side(sd[f'{side}_embed.weight'], idx, sd['prototypes'])
    return torch.relu(sd[f'{side}_embed.weight'][idx])


def combine(alg, u_repr, i_repr):
    """combine_user_item_representations (sgd_alg.py:685-688, 748-751, 818-826)."""
    if alg == 'uiprotomfs':
        (u_sim, u_proj), (i_sim, i_proj) = u_repr, i_repr
        return (u_sim.unsqueeze(-2) * i_proj).sum(dim=-1) + (u_proj.unsqueeze(-2) * i_sim).sum(dim=-1)
    return (u_repr.unsqueeze(-2) * i_repr).sum(dim=-1)


def forward(alg, sd, u, i):
    """Train-mode forward: logits [B, N]."""
    return combine(alg, representations(alg, sd, 'user', u), representations(alg, sd, 'item', i))


def scores_all(alg, sd, u, n_items):
    """eval/eval.py:205-217: the users u against every item."""
    return combine(alg, representations(alg, sd, 'user', u), representations(alg, sd, 'item', torch.arange(n_items)))


def rec_loss(kind, logits, labels):
    """train/rec_losses.py:40-83 ('bce' | 'bpr', mean) through torch's own BCE-with-logits, as the reference calls it. A zero embedding
    row gives logits of exactly 0, where the max / abs form of oracle/losses_ref.py takes another subgradient than sigmoid(x) - y."""
    if kind == 'bpr':
        logits, labels = logits[:, :1] - logits[:, 1:], torch.repeat_interleave(labels[:, 0], logits.shape[1] - 1)
    return torch.nn.BCEWithLogitsLoss(reduction='mean')(logits.flatten(), labels.flatten())


def _post_val(prototypes, entities, other):
    """The scalar entries of explanations/utils.py:260-300 with sim_func = compute_cosine_sim, the full (P + n)^2 matrix as in the
    reference."""
    n = len(prototypes)
    if len(entities) >= MAX_ENTITIES:
        entities = entities[torch.randperm(len(entities))[:MAX_ENTITIES]]
    both = torch.cat([prototypes, entities])
    sim_mtx = cosine_sim(both, both)
    e2p = sim_mtx[n:, :n]
    return {'avg_pairwise_proto_sim': ((torch.tril(sim_mtx[:n, :n], diagonal=-1).sum() * 2) / (n * (n - 1))).item(),
            'entity_to_proto_mean': e2p.mean(dim=-1).mean().item(), 'entity_to_proto_max': e2p.max(dim=-1).values.mean().item(),
            'entity_to_proto_min': e2p.min(dim=-1).values.mean().item(),
            'bin_weights_mean': (other != 0).sum(dim=-1).double().mean().item(), 'sum_weights_mean': other.sum(dim=-1).mean().item()}


def post_val(alg, sd):
    with torch.no_grad():
        if alg == 'uprotomfs':
            return _post_val(sd['prototypes'], sd['user_embed.weight'], torch.relu(sd['item_embed.weight']))
        if alg == 'iprotomfs':
            return _post_val(sd['prototypes'], sd['item_embed.weight'], torch.relu(sd['user_embed.weight']))
        u_table, i_table = sd['uprotomfs.user_embed.weight'], sd['iprotomfs.item_embed.weight']
        u = _post_val(sd['uprotomfs.prototypes'], u_table, torch.relu(i_table @ sd['i_to_u_proj.weight'].T))
        i = _post_val(sd['iprotomfs.prototypes'], i_table, torch.relu(u_table @ sd['u_to_i_proj.weight'].T))
        return {**{'user_' + k: v for k, v in u.items()}, **{'item_' + k: v for k, v in i.items()}}
