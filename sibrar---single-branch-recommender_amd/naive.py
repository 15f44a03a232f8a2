"""PopularItems and RandomItems (algorithms/naive_algs.py:11-60): the two baselines every results table of the reference is read against,
behind the reference's ``RecommenderAlgorithm`` surface (algorithms/base_classes.py:12-51).

Neither has anything to fit. ``PopularItems`` scores item i with ``pop_distribution[i]`` for every user; ``RandomItems`` scores (u, i) with
a uniform draw. Both answer the hooks ``evaluate_recommender_algorithm`` calls as the fit-matrix models do (user side = the ids, item side
= the 1-tuple of item ids, ``combine_user_item_representations`` returns real [B, I] rows), so they run through the ``fp32`` route, unsharded
on every rank under ``shard_items=True``.

``PopularItems`` also offers ``topk_lists``: since every user has the same row, a user's list is the shared ranking minus the user's
exclusions, and ``ops.shared_rank_topk`` (csrc/shared_rank.hip) reads about ``k + |excl(u)|`` entries per user instead of writing,
masking and selecting from a [chunk, items] matrix of identical rows. The evaluation loop takes a model's ``topk_lists`` when it has one.

Deliberate differences from the reference: scores are fp32 (the reference keeps ``pop_distribution`` in float64); ties are canonical —
equal scores go in ascending item position, where the reference's ``torch.topk`` leaves them open; the slots behind a user's last scoreable
item hold (-inf, -1); ``RandomItems`` is seeded and counter-based — ``U(seed, user, item)`` from Philox4x32-10 (``ops.uniform_rows``) —
where the reference draws ``torch.rand(i_idxs.shape)`` from the CPU's global generator, so that its lists depend on the batch size, the
order of the batches and whatever drew before. Here a list does not depend on the chunking of the users, and two runs give the same lists.
"""
from __future__ import annotations

import logging
from abc import ABC, abstractmethod

import numpy as np
import torch

from . import ops


class _NaiveAlgorithm(ABC):
    """What the two share: nothing to fit, nothing to save, and the evaluation hooks of ``ResidentMatrixAlgorithm``."""

    def __init__(self, device=None):
        self.device = torch.device(device or 'cuda')

    def to(self, device):
        self.device = torch.device(device)
        return self

    def eval(self):
        return self

    def train(self, mode: bool = True):
        return self

    def save_model_to_path(self, path: str):
        pass

    def load_model_from_path(self, path: str):
        pass

    @abstractmethod
    def _score_items(self, u: torch.Tensor, items: torch.Tensor) -> torch.Tensor:
        """-> float32 [len(u), I] for ``items`` [I], [len(u), n] for ``items`` [len(u), n]; both on the model's device"""

    def get_user_representations(self, u_idxs: torch.Tensor):
        return torch.as_tensor(u_idxs).long().to(self.device)

    def get_item_representations(self, i_idxs: torch.Tensor):
        return (torch.as_tensor(i_idxs).long().to(self.device),)

    @torch.no_grad()
    def combine_user_item_representations(self, u_repr, i_repr) -> torch.Tensor:
        """-> float32 [len(u_repr), len(items)]: the users' score rows over the named item columns, real memory (the evaluation masks
        them in place)"""
        return self._score_items(u_repr, i_repr[0])

    @torch.no_grad()
    def predict(self, u_idxs: torch.Tensor, i_idxs: torch.Tensor) -> torch.Tensor:
        """u_idxs [batch_size], i_idxs [batch_size, n] -> scores [batch_size, n]"""
        return self._score_items(self.get_user_representations(u_idxs), torch.as_tensor(i_idxs).long().to(self.device))


class PopularItems(_NaiveAlgorithm):
    """algorithms/naive_algs.py:35-60. ``pop_distribution``: array of shape (n_items,), an item's popularity value. The values are kept as
    fp32 (the reference: float64). Rounding is monotone, so no strict order is ever inverted; it can only add ties, and only between values
    less than one fp32 spacing (2^-23, relatively) apart. With the reference's formula (data/dataset.py:357-359: interaction counts over
    their total) distinct counts c < c' differ relatively by at least 1 / c', so the fp32 scores keep every strict order and add no ties
    while no item has 2^23 interactions or more. Non-finite values or anything but a vector raise ``ValueError``."""

    def __init__(self, pop_distribution: np.ndarray, device=None):
        super().__init__(device)
        pop = pop_distribution.detach().cpu().numpy() if torch.is_tensor(pop_distribution) else np.asarray(pop_distribution)
        if pop.ndim != 1 or pop.dtype.kind not in 'fiub':
            raise ValueError(f'pop_distribution must be a numeric vector of shape (n_items,), got {pop.dtype} {pop.shape}')
        if not np.isfinite(pop.astype(np.float64)).all():
            raise ValueError('pop_distribution holds non-finite values')
        with np.errstate(over='ignore'):
            pop32 = pop.astype(np.float64).astype(np.float32)
        if not np.isfinite(pop32).all():
            raise ValueError('pop_distribution holds values beyond the fp32 range')
        self.pop_distribution = torch.from_numpy(pop32)               # float32 [n_items]; moved to the model's device on first use
        self._ranking = None                                          # (items, score, order) of the last catalogue topk_lists saw
        self.name = 'PopularItems'
        logging.info(f'Built {self.name} module')

    @property
    def n_items(self) -> int:
        return int(self.pop_distribution.numel())

    def _pop(self) -> torch.Tensor:
        if self.pop_distribution.device != self.device:
            self.pop_distribution = self.pop_distribution.to(self.device)
            self._ranking = None
        return self.pop_distribution

    def _score_items(self, u, items):
        row = self._pop()[items]                                      # naive_algs.py:49
        return row.expand(u.numel(), row.numel()).contiguous() if items.dim() == 1 else row

    @torch.no_grad()
    def topk_lists(self, u_idxs: torch.Tensor, items: torch.Tensor, excl_indptr: torch.Tensor, excl_indices: torch.Tensor, k: int):
        """-> (val float32 [B, k], idx int32 [B, k]): per user the ``k`` most popular of ``items`` (int64 [I], the split's item ids) that
        the user's row of the exclusion CSR (columns = positions in ``items``) does not hold: positions in ``items``, best first, equal
        scores in ascending position, (-inf, -1) behind a user's last scoreable item. The ranking of ``items`` is made once and kept for
        the next call with the same ``items``."""
        items = torch.as_tensor(items).long().to(self.device)
        kept = self._ranking
        if kept is None or kept[0].device != items.device or not (kept[0] is items or (kept[0].shape == items.shape and torch.equal(kept[0], items))):
            score = self._pop()[items].contiguous()
            kept = self._ranking = (items, score, ops.shared_ranking(score))
        u = torch.as_tensor(u_idxs).long().to(self.device).contiguous()
        return ops.shared_rank_topk(kept[2], kept[1], u, excl_indptr, excl_indices, k)

    @staticmethod
    def build_from_conf(conf: dict, dataset):
        """naive_algs.py:58-60; a dataset without ``pop_distribution`` gets the reference's formula (data/dataset.py:357-359): the column
        sums of ``user_sampling_matrix`` over their total, in float64"""
        pop = getattr(dataset, 'pop_distribution', None)
        if pop is None:
            item_popularity = np.array(dataset.user_sampling_matrix.sum(axis=0), dtype=np.float64).flatten()
            with np.errstate(invalid='ignore', divide='ignore'):
                pop = item_popularity / item_popularity.sum()
        return PopularItems(pop)


class RandomItems(_NaiveAlgorithm):
    """algorithms/naive_algs.py:11-32, as a pure function: the score of (u, i) is ``U(seed, u, i)`` in [0, 1) (``ops.uniform_rows``), whatever
    the batch it is asked in. ``seed``: an integer in [0, 2^64)."""

    def __init__(self, seed: int = 0, device=None):
        super().__init__(device)
        if isinstance(seed, bool) or int(seed) != seed or not 0 <= seed < 1 << 64:
            raise ValueError(f'seed={seed!r} must be an integer in [0, 2^64)')
        self.seed = int(seed)
        self.name = 'RandomItems'
        logging.info(f'Built {self.name} module')

    def _score_items(self, u, items):
        if items.dim() == 2 and items.shape[0] != u.numel():
            raise ValueError(f'{self.name}: {items.shape[0]} item rows for {u.numel()} users')
        n = int(items.max()) + 1 if items.numel() else 0              # the users' rows over the item ids [0, n), then the named columns
        rows = ops.uniform_rows(self.seed, u.contiguous(), n)
        if items.dim() == 1:
            whole = items.numel() == n and bool((items == torch.arange(n, device=items.device)).all())
            return rows if whole else rows[:, items]
        return torch.gather(rows, 1, items)

    @staticmethod
    def build_from_conf(conf: dict, dataset=None):
        """naive_algs.py:30-32, with the optional ``conf['seed']``"""
        return RandomItems((conf or {}).get('seed', 0))
