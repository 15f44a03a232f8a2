"""Plain-torch CPU restatement of DeepMatrixFactorization (algorithms/sgd_alg.py:1141-1242) over a flat state_dict — a test helper,
not a test. It computes in the dtype of the state_dict it is given, so a float64 copy of the parameters serves as the truth.

    sd      {'user_nn.layers.linear_0.weight': ..., ...}     (modules/polylinear.py:39-77 names)
    inter   scipy CSR [n_users, n_items], inter_t its transpose (data/dataset.py:260-273: get_*_interaction_vectors)
"""
import numpy as np
import torch


def _rows(matrix, idx, dtype, normalize):
    """dataset.get_*_interaction_vectors(idx).float() (+ sgd_alg.py:1211-1213 / 1226-1228)."""
    flat = np.asarray(idx).reshape(-1)
    x = torch.from_numpy(np.asarray(matrix[flat].todense())).to(dtype)
    if normalize:
        x = x / torch.linalg.vector_norm(x, dim=-1, keepdim=True).clamp(min=1e-8)
    return x.reshape(*np.asarray(idx).shape, x.shape[-1])


def _tower(sd, prefix, x, use_output_activation_fn):
    """PolyLinear(layers, activation_fn=ReLU, output_fn=ReLU | None) — sgd_alg.py:1179-1181."""
    n = sum(1 for k in sd if k.startswith(f'{prefix}.layers.linear_') and k.endswith('.weight'))
    for l in range(n):
        x = torch.nn.functional.linear(x, sd[f'{prefix}.layers.linear_{l}.weight'], sd[f'{prefix}.layers.linear_{l}.bias'])
        if l < n - 1 or use_output_activation_fn:
            x = torch.relu(x)
    return x


def representations(sd, side, matrix, idx, normalize_interactions=False, normalize_representations=False,
                    use_output_activation_fn=False):
    """sgd_alg.py:1208-1236; side = 'user' (matrix = inter) or 'item' (matrix = inter_t)."""
    dtype = sd[f'{side}_nn.layers.linear_0.weight'].dtype
    x = _tower(sd, f'{side}_nn', _rows(matrix, idx, dtype, normalize_interactions), use_output_activation_fn)
    if normalize_representations:
        x = x / torch.linalg.vector_norm(x, dim=-1, keepdim=True).clamp(min=1e-8)
    return x


def combine(u_repr, i_repr, mu):
    """sgd_alg.py:1238-1242."""
    sim = torch.nn.CosineSimilarity(dim=-1)(u_repr[:, None, :], i_repr)
    sim = sim.clone()
    sim[sim < mu] = mu
    return sim


def forward(sd, inter, inter_t, u, i, mu=1e-6, **kw):
    """sgd_alg.py:1193-1197: logits [B, N] of a batch u [B], i [B, N]."""
    return combine(representations(sd, 'user', inter, u, **kw), representations(sd, 'item', inter_t, i, **kw), mu)


def scores_all(sd, inter, inter_t, u, mu=1e-6, **kw):
    """eval/eval.py:205-217: the users u against every item."""
    n_items = inter.shape[1]
    return combine(representations(sd, 'user', inter, u, **kw), representations(sd, 'item', inter_t, np.arange(n_items), **kw), mu)


MODEL_KW = ('normalize_interactions', 'normalize_representations', 'use_output_activation_fn')


def split_kwargs(kwargs):
    """constructor kwargs of a fixture case -> (mu, restatement kwargs)"""
    return kwargs.get('mu', 1e-6), {k: kwargs[k] for k in MODEL_KW if k in kwargs}
