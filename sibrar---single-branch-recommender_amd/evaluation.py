"""Full-catalogue evaluation with the reference's hooks: ``FullEvaluator`` and ``evaluate_recommender_algorithm``
(eval/eval.py:20-168, 171-227).

The reference scores a user batch against all items (``einsum('be,ce->bc')``), sets ``out[exclude_data[u]] = -inf`` from a
host-densified CSR mask, and hands the dense [Bu, I_s] logits plus dense label rows to the third-party ``rmet.calculate``.
Here the exclusion CSR and the label CSR are resident on the device; per user batch the engine runs either
  * ``scorer='fp32'``      : fp32-MFMA GEMM -> CSR mask kernel -> exact radix-select top-k, or
  * ``scorer='fp16_fused'``: the fused fp16-MFMA score+mask+top-k kernel (scores never written), or
  * ``scorer='fp32_fused'``: the same fusion with fp32-class products (fp32 user rows and the item matrix split once into three
    exact bf16 planes, six bf16-MFMA partial products per score, fp32 accumulation): the fp32 route's ranking without its score
    matrix; D in {64, 128} (D = 256 with ``fused_max_d=256``) and finite item values, anything else falls back to ``'fp32'``,
both fused routes for lists up to ``fused_max_k`` entries (default 32; up to 128 on request: the wide kernels), longer ones fall back,
followed by the ranking-metric kernel (NDCG / recall / precision as defined in eval/metrics.py:4-105; ``rmet`` itself is
absent offline, so w.r.t. ``rmet`` the metric arithmetic is parity-unpinned) and, when ``config.metrics`` names one of them, by the
rank-position kernel (``dcg``, ``ap``, ``rr``: defined in include/sibrar_hip.h at ``sbr_rank_metrics_pos``, equally unpinned against
``rmet``). ``eval_batch`` keeps the reference's
dense-logits entry point for callers that already hold a score matrix. A model with a callable ``topk_lists`` (``PopularItems``: one
score row for all users) hands over a chunk's lists itself and none of the three routes runs.

``gather_recommender_algorithm_results`` / ``Gatherer`` (eval/eval.py:230-333) dump the per-user top-``max(top_k)`` lists next to the
metrics; they run the same scoring loop as the evaluation.

``paired_significance`` (eval/stat_tests.py:15-38) is the paired t-test with Bonferroni correction over the per-user arrays that
``get_results(return_raw_results=True)`` returns; it runs on the host.
"""
from __future__ import annotations

import logging
import pickle
import re
from collections import defaultdict
from typing import Optional, Sequence

import numpy as np
import scipy.sparse as sp
import torch

from . import ops, parallel

DEFAULT_METRICS = ('ndcg', 'precision', 'recall', 'f_score', 'hitrate', 'coverage')      # what an evaluator without a config reports
POSITION_METRICS = ('dcg', 'ap', 'rr')             # sbr_rank_metrics_pos, in the order of its output; computed only when asked for
SUPPORTED_METRICS = DEFAULT_METRICS + POSITION_METRICS


RANK_METRIC_MAX_KS = 8            # cut-offs per sbr_rank_metrics / sbr_rank_metrics_pos launch (METRIC_MAX_KS in csrc/topk.hip)
_OWN_LISTS_LOGGED = set()         # model classes whose use of ``topk_lists`` has been logged (once per class)


class _Cfg:
    """The fields of the reference's EvalConfig (data/config_classes.py:183-198) with its defaults."""

    def __init__(self, top_k=(1, 3, 5, 10, 20, 50, 100), metrics=DEFAULT_METRICS, calculate_std=True,
                 calculate_group_metrics=False, user_group_features=None):
        self.top_k, self.metrics, self.calculate_std = list(top_k), list(metrics), calculate_std
        self.calculate_group_metrics, self.user_group_features = calculate_group_metrics, user_group_features


def natural_key(s: str):
    """Sort key of ``natsorted`` (eval/eval.py:160; natsort's default: unsigned integers inside a string compare as numbers,
    so 'ndcg@3' < 'ndcg@10' < 'ndcg@10_std'). natsort itself is not a dependency of this package."""
    return [int(t) if t.isdigit() else t for t in re.split(r'(\d+)', s)]


def _cfg_get(cfg, name, default=None):
    return cfg.get(name, default) if isinstance(cfg, dict) else getattr(cfg, name, default)


def _is_categorical(feature) -> bool:
    t = getattr(getattr(feature, 'feature_definition', None), 'type', None)
    return str(getattr(t, 'value', t)).lower() == 'categorical'


def _csr_to_device(m: sp.spmatrix, device):
    m = sp.csr_matrix(m)
    m.sort_indices()
    m.eliminate_zeros()
    return (torch.from_numpy(m.indptr.astype(np.int64)).to(device), torch.from_numpy(m.indices.astype(np.int32)).to(device))


class FullEvaluator:
    """eval/eval.py:20-168 — accumulates per-user metric arrays over batches; ``get_results`` averages them."""

    def __init__(self, config=None, evaluator_name: str = None, dataset=None):
        self.config = config if config is not None else _Cfg()
        self.name = evaluator_name
        self.dataset = dataset
        invalid = set(self.config.metrics) - set(SUPPORTED_METRICS)
        if invalid:
            raise ValueError(f'Metric(s) {invalid} are not supported. Select metrics from {SUPPORTED_METRICS}.')
        self._ks = sorted(set(int(k) for k in self.config.top_k))
        self._labels_dev = None
        self._user_features = self._determine_user_features()
        self._group_maps = {}            # feature name -> (int32 id -> category map on the device, labels)
        self._warned = False
        self._reset()

    def _determine_user_features(self):
        """eval/eval.py:74-92: the categorical user features for which group-wise metrics are calculated (None: no groups)."""
        if not _cfg_get(self.config, 'calculate_group_metrics', False):
            return None
        ds = self.dataset
        feats = getattr(ds, 'user_features', None)
        if ds is None or feats is None:
            raise ValueError('calculate_group_metrics needs the dataset (its categorical user features define the groups)')
        wanted = _cfg_get(self.config, 'user_group_features')
        if wanted is not None:
            names = getattr(ds, 'user_feature_names', None)
            for feature_name in wanted:
                if feature_name not in (names if names is not None else feats):
                    raise ValueError(f'Dataset does not contain user feature "{feature_name}". '
                                     f'Check config whether features are loaded or set to "None" to use'
                                     f'all available categorical features.')
                if not _is_categorical(feats[feature_name]):
                    raise ValueError(f'User feature "{feature_name}" is not categorical.')
            return list(wanted)
        defs = getattr(ds, 'user_feature_definitions', None)
        if defs is not None:
            return [d.name for d in defs if str(getattr(d.type, 'value', d.type)).lower() == 'categorical']
        # features the model adds itself (sgd_alg.py:2021-2032) are not feature definitions of the dataset
        return [n for n, f in feats.items() if _is_categorical(f) and n not in ('user_embedding', 'interactions')]

    def _reset(self):
        self._results = defaultdict(list)
        self._topk = []
        self._groups = defaultdict(list)     # feature name -> per batch int32 category of every evaluated user

    def _key(self, metric, k):
        base = f'{metric}@{k}'
        return f'{self.name}/{base}' if self.name else base

    def _labels(self, device):
        if self._labels_dev is None or self._labels_dev[0].device != torch.device(device):
            ds = self.dataset
            cached = getattr(ds, '_labels_dev', None)          # evaluators come and go (one per evaluation), the split does not
            if cached is None or cached[0].device != torch.device(device):
                lab = sp.csr_matrix(ds.user_sampling_matrix)[:, np.asarray(ds.items_in_split)]
                cached = _csr_to_device(lab, device)
                try:
                    ds._labels_dev = cached
                except Exception:
                    pass
            self._labels_dev = cached
        return self._labels_dev

    def eval_topk(self, u_idxs: torch.Tensor, topk_idx: torch.Tensor):
        """Engine entry point: per-user top-k item positions (int32 [Bu, kmax], kmax >= max(top_k))."""
        kmax = topk_idx.shape[1]
        ks = [k for k in self._ks if k <= kmax]
        if len(ks) < len(self._ks) and not self._warned:
            self._warned = True
            logging.warning(f'FullEvaluator: cut-offs {[k for k in self._ks if k > kmax]} exceed the {kmax} ranked items per user '
                            f'(catalogue of the split or the scorer\'s list length); their metrics are not reported')
        indptr, indices = self._labels(topk_idx.device)
        topk_idx, u_long = topk_idx.contiguous(), u_idxs.long().contiguous()
        # [3, n_ks, Bu]; the kernel takes up to RANK_METRIC_MAX_KS cut-offs per launch
        m = torch.cat([ops.rank_metrics(topk_idx, u_long, indptr, indices, ks[c:c + RANK_METRIC_MAX_KS])
                       for c in range(0, len(ks), RANK_METRIC_MAX_KS)], dim=1) if ks else None
        wanted_pos = [name for name in POSITION_METRICS if name in self.config.metrics]
        mp = torch.cat([ops.rank_metrics_pos(topk_idx, u_long, indptr, indices, ks[c:c + RANK_METRIC_MAX_KS])
                        for c in range(0, len(ks), RANK_METRIC_MAX_KS)], dim=1) if ks and wanted_pos else None
        for name in (self._user_features or ()):
            gmap = self._group_map(name, topk_idx.device)[0]
            # ids beyond the map (only possible when the dataset does not state n_users): category -1 -> KeyError in get_results
            self._groups[name].append(torch.where(u_long < gmap.numel(), gmap[u_long.clamp(max=max(gmap.numel() - 1, 0))],
                                                  torch.full_like(u_long, -1, dtype=torch.int32)) if gmap.numel() else
                                      torch.full_like(u_long, -1, dtype=torch.int32))
        for qi, k in enumerate(ks):
            nd, rc, pr = m[0, qi], m[1, qi], m[2, qi]
            if 'ndcg' in self.config.metrics:
                self._results[self._key('ndcg', k)].append(nd)
            if 'recall' in self.config.metrics:
                self._results[self._key('recall', k)].append(rc)
            if 'precision' in self.config.metrics:
                self._results[self._key('precision', k)].append(pr)
            if 'hitrate' in self.config.metrics:
                self._results[self._key('hitrate', k)].append((pr > 0).float())
            if 'f_score' in self.config.metrics:
                den = pr + rc
                self._results[self._key('f_score', k)].append(torch.where(den > 0, 2 * pr * rc / den.clamp_min(1e-30), den))
            for name in wanted_pos:
                self._results[self._key(name, k)].append(mp[POSITION_METRICS.index(name), qi])
        if 'coverage' in self.config.metrics:
            self._topk.append(topk_idx)

    def _group_map(self, name, device):
        """Resident ``user id -> category`` map of one categorical user feature (replaces the per-batch host lookup
        ``user_feature[u_idxs]`` + ``get_labels`` of eval/eval.py:110-113) and the group labels (lower-cased strings)."""
        got = self._group_maps.get(name)
        if got is None or got[0].device != torch.device(device):
            f = self.dataset.user_features[name]
            vals = np.asarray(f.values).astype(np.int64).reshape(-1)
            ids = np.asarray(getattr(f, '_indices', np.arange(len(vals)))).astype(np.int64)
            # one entry per user id the evaluation can name (ids without a value of this feature stay -1 and raise KeyError in
            # get_results, as eval/eval.py:110-113 does on the host) — never a device gather past the end of the map
            n_ids = max(int(ids.max()) + 1 if len(ids) else 0, int(getattr(self.dataset, 'n_users', 0) or 0))
            cat = np.full(n_ids, -1, dtype=np.int32)
            cat[ids] = vals
            uniq = getattr(f, 'unique_values', None)
            n_cat = int(vals.max()) + 1 if len(vals) else 0
            labels = [uniq[c] if uniq is not None and c < len(uniq) else c for c in range(n_cat)]
            labels = [lbl.lower() if isinstance(lbl, str) else lbl for lbl in labels]
            got = self._group_maps[name] = (torch.from_numpy(cat).to(device), labels)
        return got

    def eval_batch(self, u_idxs: torch.Tensor, logits: torch.Tensor, y_true: torch.Tensor = None):
        """Reference entry point (eval.py:121-138): dense [Bu, I_s] logits (already masked). ``y_true`` is ignored when the
        evaluator was built with a dataset (labels come from the resident CSR); without a dataset the dense rows are used."""
        if y_true is not None and logits.shape != y_true.shape:
            raise AttributeError(f'logits and true labels must have the same shape ({logits.shape} != {y_true.shape})')
        if len(u_idxs) != len(logits):
            raise AttributeError('assumed batch size is not equal for user indices, logits and true labels')
        kmax = min(max(self._ks), logits.shape[1])
        _, idx = ops.topk_rows(logits.float().contiguous(), kmax)
        if self.dataset is None:
            lab = sp.csr_matrix(y_true.detach().cpu().numpy() > 0)
            self._labels_dev = _csr_to_device(lab, logits.device)
            self.eval_topk(torch.arange(len(u_idxs), device=logits.device), idx)
            self._labels_dev = None
        else:
            self.eval_topk(u_idxs, idx)

    def get_results(self, return_raw_results: bool = False):
        keys = list(self._results)
        if keys:                       # one device -> host transfer for all metrics instead of one (and one sync) per metric
            stacked = torch.stack([torch.cat(self._results[k]).float() for k in keys]).cpu().numpy()
            raw = {k: stacked[i] for i, k in enumerate(keys)}
        else:
            raw = {}
        # group-wise metrics (eval/eval.py:106-119): the same per-user values, restricted to the users of each category of
        # each group feature. Key layout '{evaluator/}{feature}_{label}/{metric}@{k}' as rmet.calculate_for_feature
        # flattens it — rmet is absent offline, so the key layout is parity-unpinned (the values are not: a group's array is
        # the overall array under a mask).
        for name in (self._user_features or ()):
            if not self._groups[name] or not raw:
                continue
            cats = torch.cat(self._groups[name]).cpu().numpy()
            labels = self._group_maps[name][1]
            prefix = f'{self.name}/' if self.name else ''
            for c in np.unique(cats):
                if c < 0:
                    raise KeyError(f'user without a value of group feature "{name}"')
                sel = cats == c
                for k in keys:
                    raw[f'{prefix}{name}_{labels[c]}/{k[len(prefix):]}'] = raw[k][sel]
        metrics = {k: float(v.mean()) for k, v in raw.items()}
        if _cfg_get(self.config, 'calculate_std', False):
            metrics.update({f'{k}_std': float(v.std()) for k, v in raw.items()})
        if self._topk:
            top = torch.cat(self._topk)
            n_items = self.dataset.n_items_in_split if self.dataset is not None else int(top.max()) + 1
            for k in self._ks:
                if k <= top.shape[1]:
                    # distinct recommended items: mark-and-count over the item range (torch.unique sorts its 2M inputs: ~0.7 ms
                    # per cut-off on c2); empty slots (-1: users with fewer than k scoreable items) are not items
                    ids = top[:, :k].reshape(-1).long()
                    ids = ids[ids >= 0]
                    seen = torch.zeros(max(int(n_items), int(ids.max()) + 1 if ids.numel() else 1), dtype=torch.bool, device=top.device)
                    seen[ids] = True
                    metrics[self._key('coverage', k)] = int(seen.sum()) / n_items
        metrics = {k: metrics[k] for k in sorted(metrics, key=natural_key)}      # natsorted (eval/eval.py:160)
        self._reset()
        return (metrics, raw) if return_raw_results else metrics


def evaluate_recommender_algorithm(alg, eval_loader, evaluator: FullEvaluator, device='cuda', return_raw=False, verbose=False,
                                   scorer: str = 'fp32', user_chunk: Optional[int] = None, shard_items: bool = False,
                                   fused_max_k: int = 32, fused_max_d: int = 128):
    """eval/eval.py:171-227 (SGD branch :203-222). ``eval_loader`` only has to expose ``dataset`` and ``batch_size``.

    ``fused_max_k`` (32 .. 128, anything else raises ValueError): the longest list the fused routes may serve. With the default an
    evaluation whose largest cut-off is above 32 takes the fp32 route, as it always did; with 128 it stays on the requested fused route
    (the wide kernels) up to a largest cut-off of 128.

    ``fused_max_d`` (128 or 256, anything else raises ValueError): the widest representation ``scorer='fp32_fused'`` may serve. With the
    default a 256-wide model takes the fp32 route, as it always did; with 256 it is scored by ``ops.score_topk_f32s_d256``.

    The users are scored in engine-sized chunks, not in the loader's batches: per-user results do not depend on the grouping,
    and the reference's default evaluation batch (256 users) leaves the GPU idle — the fused kernel assigns 448 users to a workgroup and every workgroup streams the whole catalogue, so they want >= 57k users per launch (measured on
    c2, 100k users, first kernel: 975 ms with 256-user batches, 37 ms with 8192, 12 ms in one launch); the fp32 path is bounded by the [chunk, items] score
    matrix it materialises. ``user_chunk`` overrides the choice.

    **Item-sharded on request** (``shard_items=True`` under an initialised process group; new: SURVEY.md 8(e), BASELINE configs[4] —
    the reference has no multi-GPU path; ``Trainer.val`` opts in, a rank-0-only evaluation simply does not): EVERY rank of the group
    must make the same call on the same split (the routine runs collectives; the ranks first check that they agree on the split's item
    and user lists and raise otherwise instead of hanging or merging lists of different users). Rank r computes the representations of items [lo_r, hi_r) of the split only and scores every user chunk against them
    (fused kernel with ``item_offset``, or fp32 GEMM + shard-aware mask + top-k); the per-shard ``[Bu, k]`` (score, item position)
    lists are all-gathered and merged exactly (``parallel.all_gather_topk`` -> ``sbr_merge_topk``: score desc, index asc), and every
    rank feeds the merged lists to its evaluator — all ranks return the same metrics as a one-rank evaluation. Models whose item side
    is more than one matrix (biases) score unsharded on every rank."""
    fused_max_k, fused_max_d = ops.check_fused_max_k(fused_max_k), ops.check_fused_max_d(fused_max_d)
    _score_split(alg, eval_loader, evaluator, device, scorer, user_chunk, shard_items, fused_max_k, None, fused_max_d)
    return evaluator.get_results(return_raw_results=return_raw)


def _score_split(alg, eval_loader, evaluator: FullEvaluator, device, scorer, user_chunk, shard_items, fused_max_k, sink, fused_max_d=128):
    """The scoring loop of ``evaluate_recommender_algorithm`` and ``gather_recommender_algorithm_results``: every user chunk's top-k
    lists go to the evaluator and, when given, to ``sink(first row of the chunk, u_idxs, scores [Bu, k], item positions [Bu, k])``.
    Returns the list length k = min(max(top_k), items in the split)."""
    dataset = eval_loader.dataset
    for attr in ('items_in_split', 'users_in_split', 'exclude_data'):
        if not hasattr(dataset, attr):
            raise ValueError("Dataset underlying loader must be of type 'FullEvaluatorDataset'")
    alg.eval()
    kmax = max(evaluator._ks)
    with torch.no_grad():
        items = torch.as_tensor(np.asarray(dataset.items_in_split)).to(device)
        n_split = int(items.shape[0])
        world = parallel.world_size() if (shard_items and parallel.is_distributed()) else 1
        lo, hi = 0, n_split
        sharded = False
        users = np.asarray(dataset.users_in_split)
        if world > 1:
            # all ranks must be evaluating the same split: (items, users, sum of user ids, sum of item ids) agree or nobody shards
            fp = torch.tensor([n_split, len(users), int(users.astype(np.int64).sum()), int(items.sum())], device=device, dtype=torch.int64)
            fp_lo, fp_hi = fp.clone(), fp.clone()
            torch.distributed.all_reduce(fp_lo, op=torch.distributed.ReduceOp.MIN)
            torch.distributed.all_reduce(fp_hi, op=torch.distributed.ReduceOp.MAX)
            if not bool((fp_lo == fp_hi).all()):
                raise ValueError(f'evaluate_recommender_algorithm(shard_items=True): the ranks evaluate different splits '
                                 f'(items / users / id sums: this rank {fp.tolist()}, min {fp_lo.tolist()}, max {fp_hi.tolist()})')
        if world > 1 and (world - 1) * (-(-n_split // world)) < n_split:      # every rank gets a non-empty shard
            rank = torch.distributed.get_rank()
            lo, hi = parallel.item_shard(n_split, rank, world)
            probe = alg.get_item_representations(items[lo:hi])                # this rank's item shard only
            sharded = torch.is_tensor(probe)
            i_repr = probe if sharded else alg.get_item_representations(items)
            if not sharded:
                lo, hi = 0, n_split
        else:
            i_repr = alg.get_item_representations(items)                      # once: [I_s, D] (or a tuple: embeddings, biases, ...)
        plain = torch.is_tensor(i_repr)       # models whose item side is more than one matrix score through their own combine
        i_dev = i_repr.device if plain else i_repr[0].device
        kmax = min(kmax, n_split)
        excl = getattr(dataset, '_excl_dev', None)
        if excl is None or excl[0].device != i_dev:
            excl = _csr_to_device(dataset.exclude_data, i_dev)
            try:
                dataset._excl_dev = excl
            except Exception:
                pass
        bs = int(getattr(eval_loader, 'batch_size', 256) or 256)
        if scorer not in ('fp32', 'fp16_fused', 'fp32_fused'):
            raise ValueError(f'unknown scorer {scorer!r}')
        # a model that makes its own lists (PopularItems: every user has the same score row, so a list is the shared ranking minus the
        # user's exclusions) provides ``topk_lists(u_idxs, items, excl_indptr, excl_indices, k) -> (val, idx)`` in the conventions of the
        # routes below; unsharded evaluations take a chunk's lists from it and ``scorer`` has nothing to choose. Models without the hook
        # are untouched.
        own_lists = getattr(alg, 'topk_lists', None)
        own_lists = own_lists if callable(own_lists) and not sharded else None
        if own_lists is not None:
            if type(alg) not in _OWN_LISTS_LOGGED:
                _OWN_LISTS_LOGGED.add(type(alg))
                logging.info(f'{getattr(alg, "name", type(alg).__name__)} makes its own top-k lists (topk_lists): scorer={scorer!r} is not used')
            scorer = 'fp32'
        # the fused routes: (item operand made once per call, user operand made per chunk, call). fp16_fused is built for D in
        # {64, 128, 256}, fp32_fused for D in {64, 128} (D = 256 has kernels of its own, used with fused_max_d = 256); both serve lists up to
        # fused_max_k entries (ops.score_topk_fused_supported). Everything else — larger cut-offs (the reference's default evaluator
        # asks for top-100: fused only with fused_max_k >= 100), tuple item sides — takes the exact fp32 GEMM + radix-select path.
        fused_routes = {
            'fp16_fused': (ops.cast_f16, ops.cast_f16, ops.score_topk_f16),
            'fp32_fused': (ops.split_bf16x3, lambda u: u, ops.score_topk_f32s),
        }
        # a tuple item side is scored by the fused kernels only if the model names the one matrix its dot-product score uses (ACF:
        # ``fused_score_transform()[0]`` picks i_repr[0]); every other tuple model scores through its own combine on the fp32 path
        # a model with a plain item side whose score is NOT the dot product of the two representations (NeuMF with MLP layers: a learned
        # non-linear function of the pair) says so with ``dot_product_score = False`` and is scored by its own combine on the fp32 path
        if scorer in fused_routes and not getattr(alg, 'dot_product_score', True):
            logging.info(f'{scorer} scorer: the score of {getattr(alg, "name", type(alg).__name__)} is not a dot product, using the fp32 path')
            scorer = 'fp32'
        fused_items = i_repr if plain else None
        if not plain and scorer in fused_routes and hasattr(alg, 'fused_score_transform'):
            pick = alg.fused_score_transform()[0]
            picked = pick(i_repr) if pick is not None else None
            fused_items = picked if torch.is_tensor(picked) else None
        if scorer in fused_routes and (fused_items is None or not ops.score_topk_fused_supported(scorer, int(fused_items.shape[1]), kmax,
                                                                                                 fused_max_k, fused_max_d)):
            logging.info(f'{scorer} scorer: k={kmax}, item representation {"tuple" if fused_items is None else tuple(fused_items.shape)} '
                         f'outside the fused kernel, using the fp32 path')
            scorer = 'fp32'
        if scorer == 'fp32_fused' and not ops.split_bf16x3_supported(fused_items):
            # an inf / NaN (or > 3.38e38) item value splits into NaN planes: every score of that item would be NaN in the fused kernel
            logging.info('fp32_fused scorer: non-finite item representations, using the fp32 path')
            scorer = 'fp32'
        fused = scorer in fused_routes
        # a model whose score is not the plain dot product of its representations (DeepMF: a floored cosine) provides
        # ``fused_score_transform() -> (items_fn, users_fn, finish_fn)``: the fused kernels only compute dot products, so the item
        # representations pass through items_fn once, every chunk's user representations through users_fn, and every chunk's
        # (val, idx) lists through finish_fn before they are merged / evaluated / dumped. Models without the hook are untouched.
        transform = getattr(alg, 'fused_score_transform', None) if fused else None
        items_fn = users_fn = finish_fn = None
        if transform is not None:
            items_fn, users_fn, finish_fn = transform()
        if fused:
            item_operand, user_operand, score_fused = fused_routes[scorer]
            if scorer == 'fp32_fused' and int(fused_items.shape[1]) == ops.FUSED_MAX_D:
                score_fused = ops.score_topk_f32s_d256
            if items_fn is not None and plain:                      # (a tuple side has been through items_fn above)
                i_repr = fused_items = items_fn(i_repr)
            i_op = item_operand(fused_items)                        # made once per call: fp16 [I, D] or three bf16 planes [3, I, D]
        if user_chunk is not None:
            bs = int(user_chunk)
        elif fused:
            bs = max(bs, 262144)                                    # one launch for up to 256k users (fp16 rows: 64 MB at D = 128)
        else:
            bs = max(bs, min(16384, max(1, (1 << 31) // max(hi - lo, 1))))      # <= 8 GiB of fp32 scores per chunk
        for s in range(0, len(users), bs):
            u_idxs = torch.from_numpy(users[s:s + bs].astype(np.int64)).to(device)
            u_repr = alg.get_user_representations(u_idxs) if own_lists is None else None
            if own_lists is not None:
                val, idx = own_lists(u_idxs, items, excl[0], excl[1], kmax)
            elif fused and torch.is_tensor(u_repr):
                # the split's exclusion mask in the scorer's layout, built once per (user chunk, item shard, D) and kept with the
                # split like the resident CSR it is made from
                cache = getattr(dataset, '_scorer_excl', None)
                if cache is None or cache.get('csr') is not excl:
                    cache = {'csr': excl}
                    try:
                        dataset._scorer_excl = cache
                    except Exception:
                        pass
                # (the key carries a fingerprint of the chunk's user ids: a split whose users_in_split changed between two evaluations
                # must not meet the mask of the old users)
                chunk = users[s:s + bs].astype(np.int64)
                # (and the route: the two fused kernels lay the stream out for different tile widths; the list length is not part of
                # the key because a route's tile width does not depend on it: the wide kernels read the same stream)
                holder = cache.setdefault((scorer, s, int(chunk.size), int(chunk[0]), int(chunk[-1]), int(chunk.sum()), lo, hi,
                                           int(i_op.shape[-1])), ops.ScorerExclusions())
                if users_fn is not None:
                    u_repr = users_fn(u_repr)
                val, idx = score_fused(user_operand(u_repr), i_op, kmax, u_idxs, excl[0], excl[1], item_offset=lo, exclusions=holder)
                if finish_fn is not None:
                    val, idx = finish_fn(val, idx)
            else:
                out = alg.combine_user_item_representations(u_repr, i_repr)
                ops.mask_scores_(out, u_idxs, excl[0], excl[1], item_offset=lo if sharded else None)
                kl = min(kmax, hi - lo)
                val, idx = ops.topk_rows(out, kl)
                if sharded:
                    idx = idx + lo                                  # positions in items_in_split
                    if kl < kmax:                                   # a shard shorter than the list: empty slots behind its items
                        pad = (idx.shape[0], kmax - kl)
                        val = torch.cat([val, torch.full(pad, -float('inf'), device=val.device)], 1)
                        idx = torch.cat([idx, torch.full(pad, -1, device=idx.device, dtype=idx.dtype)], 1)
            if sharded:
                val, idx = parallel.all_gather_topk(val, idx, kmax)
            evaluator.eval_topk(u_idxs, idx)
            if sink is not None:
                sink(s, u_idxs, val, idx)
        if hasattr(alg, 'check_index_errors'):
            alg.check_index_errors()
    return kmax


def paired_significance(raw_by_model: dict, threshold: float = 0.05) -> dict:
    """eval/stat_tests.py:15-38 as a function: ``raw_by_model`` maps a model name to the per-user array of ONE metric (what
    ``get_results(return_raw_results=True)`` returns under that metric's key), all over the same users in the same order. The best model
    is the one with the largest mean (NaNs left out of the mean); every other model is compared with it by the paired two-sided t-test
    ``scipy.stats.ttest_rel(best, other, nan_policy='omit')`` (a pair with a NaN on either side is dropped), and the significance
    threshold is Bonferroni-corrected by the number of comparisons. ->

      ``best``        the best model's name,
      ``threshold``   ``threshold / (n_models - 1)``,
      ``p_values``    {other model: p-value},
      ``significant`` {other model: p-value <= the corrected threshold}.

    Fewer than two models or arrays of unequal lengths raise ``ValueError``. Host only."""
    from scipy import stats
    if len(raw_by_model) < 2:
        raise ValueError(f'paired_significance: {len(raw_by_model)} model(s) given, a comparison needs at least two')
    arrays = {name: np.asarray(v, dtype=np.float64).reshape(-1) for name, v in raw_by_model.items()}
    lengths = {name: a.size for name, a in arrays.items()}
    if len(set(lengths.values())) != 1:
        raise ValueError(f'paired_significance: the arrays must cover the same users, got lengths {lengths}')
    best = max(arrays, key=lambda name: np.nanmean(arrays[name]))
    corrected = threshold / (len(arrays) - 1)
    p_values = {name: float(stats.ttest_rel(arrays[best], a, nan_policy='omit').pvalue) for name, a in arrays.items() if name != best}
    return {'best': best, 'threshold': corrected, 'p_values': p_values,
            'significant': {name: bool(p <= corrected) for name, p in p_values.items()}}


class Gatherer:
    """eval/eval.py:230-258 — collects named results: arrays (numpy or torch) are appended per name and concatenated by ``gather``,
    anything else is kept as the object last added under its name."""

    def __init__(self):
        self.reset()

    def reset(self):
        self._obj_collection = {}
        self._collection = defaultdict(list)

    def add(self, name: str, values):
        if isinstance(values, torch.Tensor):
            values = values.detach().cpu().numpy()
        if isinstance(values, np.ndarray):
            self._collection[name].append(values)
        else:
            self._obj_collection[name] = values

    def gather(self) -> dict:
        results = {name: np.concatenate(parts) for name, parts in self._collection.items()}
        results.update(self._obj_collection)
        return results

    def export_pkl(self, path: str):
        with open(path, 'wb') as fh:
            pickle.dump(self.gather(), fh)


def gather_recommender_algorithm_results(alg, eval_loader, evaluator: FullEvaluator, results_path: str = None, device: str = 'cuda',
                                         verbose: bool = False, scorer: str = 'fp32', fused_max_k: int = 32,
                                         user_chunk: Optional[int] = None, fused_max_d: int = 128):
    """eval/eval.py:261-333 (SGD branch): the per-user top-k dump of a split. Returns (and pickles to ``results_path`` when given)

      ``n_users``, ``n_items``     users / items of the split,
      ``k``                        list length = max(top_k), capped at the items of the split (the reference's ``torch.topk`` raises there),
      ``topk_item_indices``        int64 [n_users, k] positions in ``items_in_split``, best first (-1 behind fewer than k scoreable items),
      ``topk_logits``              float32 [n_users, k] their scores (-inf in the empty slots),
      ``user_indices``             int64 [n_users],
      ``targets``                  int64 [n_labels, 2]: per LOADER batch (``eval_loader.batch_size`` consecutive users of the split, as the
                                   reference iterates them) ``argwhere(labels)`` = (position of the user in its batch, item position),
      ``metrics``, ``raw_metrics`` what ``evaluate_recommender_algorithm(..., return_raw=True)`` returns on the same inputs.

    The one deliberate difference: the users are SCORED in engine-sized chunks (``user_chunk``; see ``evaluate_recommender_algorithm``),
    not in the loader's batches. No result depends on that grouping — ``targets`` numbers the users by the loader's batches whatever
    the chunk. The lists leave the device once per chunk. The scoring loop is the evaluation's own (``scorer``, ``fused_max_k``, ``fused_max_d`` as there):
    the evaluator is fed from the very lists that are dumped."""
    fused_max_k, fused_max_d = ops.check_fused_max_k(fused_max_k), ops.check_fused_max_d(fused_max_d)
    dataset = eval_loader.dataset
    gatherer = Gatherer()
    bs = int(getattr(eval_loader, 'batch_size', 256) or 256)
    users = np.asarray(dataset.users_in_split)
    labels = sp.csr_matrix(dataset.user_sampling_matrix)

    def sink(first, u_idxs, val, idx):
        gatherer.add('topk_item_indices', idx.long())
        gatherer.add('topk_logits', val.float())
        gatherer.add('user_indices', u_idxs.long())
        lab = sp.csr_matrix(labels[users[first:first + len(u_idxs)]][:, np.asarray(dataset.items_in_split)])
        lab.eliminate_zeros()
        lab.sort_indices()
        rows = np.repeat(np.arange(first, first + lab.shape[0], dtype=np.int64), np.diff(lab.indptr))
        gatherer.add('targets', np.stack([rows % bs, lab.indices.astype(np.int64)], axis=1))

    k = _score_split(alg, eval_loader, evaluator, device, scorer, user_chunk, False, fused_max_k, sink, fused_max_d)
    gatherer.add('n_users', int(getattr(dataset, 'n_users_in_split', len(users))))
    gatherer.add('n_items', int(getattr(dataset, 'n_items_in_split', len(dataset.items_in_split))))
    gatherer.add('k', int(k))
    metrics, raw_metrics = evaluator.get_results(return_raw_results=True)
    gatherer.add('metrics', metrics)
    gatherer.add('raw_metrics', raw_metrics)
    if results_path is not None:
        gatherer.export_pkl(results_path)
    return gatherer.gather()
