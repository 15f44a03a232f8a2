"""Feature containers on the host side of the boundary.

``HostFeature`` is a minimal stand-in for the reference's ``data.Feature.Feature`` (data/Feature.py:27-295) with the same
attribute names, so that code written against either works; the engine itself only needs the duck-typed attributes
``feature_definition.type``, ``values``, ``_indices``, ``dim`` and ``n_unique_categories``.

``DeviceTable`` is what the engine keeps resident in HBM for one feature: the processed values (dense fp32 matrix, padded
int32 tag matrix, int32 category vector or CSR arrays) plus the int32 ``id -> row`` map that replaces
``np.vectorize(dict.__getitem__)`` of Feature.__getitem__ (data/Feature.py:146). Nothing is fetched from the host per batch.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import numpy as np
import scipy.sparse as sp
import torch
from torch import nn

KINDS = ('dense', 'csr', 'categorical', 'tag')


def _type_name(t) -> str:
    return str(getattr(t, 'value', t)).lower()


class HostFeature:
    """Processed feature values + index map, mirroring data/Feature.py. ``kind`` is one of KINDS."""

    def __init__(self, name: str, kind: str, values, indices: Optional[np.ndarray] = None, n_categories: int = None,
                 unique_values: Optional[list] = None):
        """``unique_values`` (categorical): the sorted raw values whose positions are the integer categories
        (data/Feature.py:209-218) — what ``get_labels`` maps back to; evaluation groups are named after them."""
        assert kind in KINDS
        ftype = {'dense': 'vector', 'csr': 'vector', 'categorical': 'categorical', 'tag': 'tag'}[kind]
        self.feature_definition = SimpleNamespace(name=name, type=ftype)
        self.kind = kind
        self._values = values
        n = values.shape[0]
        self._n_values = n
        self._indices = np.arange(n) if indices is None else np.asarray(indices)
        if len(self._indices) != n:
            raise ValueError(f'Provided indices must match size of supplied values ({n} != {len(self._indices)})')
        if kind in ('dense', 'csr'):
            self._dim = int(values.shape[1])
        elif kind == 'tag':
            if n_categories is None:
                raise ValueError('tag features need n_categories (number of distinct tags)')
            self._dim = int(n_categories)
        else:
            self._dim = 0
        self._n_categories = n_categories if n_categories is not None else (
            int(values.max()) + 1 if kind == 'categorical' and n > 0 else None)
        self._unique_values = list(unique_values) if unique_values is not None else None
        if self._unique_values is not None and kind == 'categorical' and self._n_categories is not None \
                and len(self._unique_values) != self._n_categories:
            raise ValueError(f'{len(self._unique_values)} unique values for {self._n_categories} categories')

    @property
    def values(self):
        return self._values

    @property
    def dim(self):
        return self._dim

    @property
    def n_values(self):
        return self._n_values

    @property
    def n_unique_categories(self):
        if self.kind != 'categorical':
            raise TypeError('Only categorical features support "n_unique_categories"')
        return self._n_categories

    @property
    def unique_values(self):
        if self.kind not in ('categorical', 'tag'):
            raise TypeError('Only categorical and tag features support "unique_values"')
        if self._unique_values is None:
            return list(range(self._n_categories if self.kind == 'categorical' else self._dim))
        return self._unique_values

    def get_labels(self, values):
        """data/Feature.py:126-128: integer categories -> raw labels."""
        if self.kind != 'categorical':
            raise TypeError('Only categorical features support "get_labels"')
        uniq = self.unique_values
        return np.array([uniq[int(v)] for v in np.asarray(values).reshape(-1)])

    def __len__(self):
        return self._n_values


def feature_kind(feature) -> str:
    """Classify a reference-like Feature object (data/Feature.py:70-87 / config_classes.py:18-34)."""
    if isinstance(feature, HostFeature):
        return feature.kind
    t = _type_name(feature.feature_definition.type)
    if t == 'categorical':
        if getattr(feature, 'dim', 0) not in (0, None):
            return 'dense'           # one-hot preprocessed categorical (Feature.py:225-228)
        return 'categorical'
    if t == 'tag':
        v = np.asarray(feature.values)
        if v.ndim == 2 and v.shape[1] == feature.dim and v.max(initial=0) <= 1 and not np.issubdtype(v.dtype, np.integer):
            return 'dense'
        return 'tag'
    if sp.issparse(feature.values):
        return 'csr'
    return 'dense'


class DeviceTable(nn.Module):
    """HBM-resident view of one feature. Buffers are non-persistent: they move with ``.to(device)`` but stay out of the
    state_dict (the reference's state_dict holds parameters and BatchNorm statistics only)."""

    def __init__(self, feature):
        super().__init__()
        self.kind = feature_kind(feature)
        values = feature.values
        ids = np.asarray(getattr(feature, '_indices', np.arange(values.shape[0])))
        n = values.shape[0]
        self.n_rows = n
        # id -> row map (identity maps are dropped)
        if n == 0 or (len(ids) == n and ids[0] == 0 and np.array_equal(ids, np.arange(n))):
            rowmap = None
        else:
            rowmap = np.full(int(ids.max()) + 1, -1, dtype=np.int32)
            rowmap[ids] = np.arange(n, dtype=np.int32)
        if self.kind == 'dense':
            v = np.asarray(values)
            if v.ndim == 1:
                v = v[:, None]
            self.dim = v.shape[1]
            self.register_buffer('values', torch.from_numpy(np.ascontiguousarray(v)).float(), persistent=False)
        elif self.kind == 'csr':
            m = sp.csr_matrix(values)
            m.sort_indices()
            self.dim = m.shape[1]
            self.register_buffer('indptr', torch.from_numpy(m.indptr.astype(np.int64)), persistent=False)
            self.register_buffer('indices', torch.from_numpy(m.indices.astype(np.int32)), persistent=False)
            data = m.data.astype(np.float32)
            self.binary = bool(np.all(data == 1))
            self.register_buffer('data', None if self.binary else torch.from_numpy(data), persistent=False)
        elif self.kind == 'categorical':
            self.dim = 0
            self.n_categories = int(feature.n_unique_categories)
            cats = np.asarray(values).astype(np.int32)
            # fold category lookup into the id map: id -> category
            rowmap = cats if rowmap is None else np.where(rowmap >= 0, cats[np.clip(rowmap, 0, None)], -1).astype(np.int32)
        else:  # tag
            self.dim = int(feature.dim)
            self.pad = int(feature.dim)
            tags = np.asarray(values).astype(np.int32)
            self.T = tags.shape[1]
            self.register_buffer('tags', torch.from_numpy(np.ascontiguousarray(tags)), persistent=False)
        self.register_buffer('rowmap', None if rowmap is None else torch.from_numpy(np.ascontiguousarray(rowmap)),
                             persistent=False)
        self._transposed = None

    def n_entries(self) -> int:
        """Stored entries of a 'csr' feature / real (non-padding) tags of a 'tag' feature (cached)."""
        if getattr(self, '_n_entries', None) is None:
            self._n_entries = int(self.indices.numel()) if self.kind == 'csr' else int((self.tags != self.pad).sum())
        return self._n_entries

    def transposed(self, n_cols=None):
        """CSR form of the TRANSPOSED matrix of a 'csr' feature, on its device: (indptr int64 [dim + 1], indices int32 [nnz] = entity
        rows, data float32 [nnz] or None). Built once, on first use (the gather form of the projector's backward pass).
        A 'tag' feature: the transpose of X[entity, tag] = 1 / (tags of the entity) — the matrix an EmbeddingBag(mean) multiplies by —
        with ``n_cols`` rows (the bag's weight rows, padding row included: it has no entries)."""
        if self.kind == 'tag':
            if self._transposed is None or self._transposed[0].device != self.tags.device or self._transposed[0].numel() != n_cols + 1:
                real = self.tags != self.pad                                                  # [n_rows, T]
                cnt = real.sum(1)
                ent = torch.arange(self.n_rows, device=self.tags.device)[:, None].expand_as(self.tags)[real]
                tag = self.tags[real].long()
                val = (1.0 / cnt.float())[ent]
                order = torch.sort(tag, stable=True).indices
                t_indptr = torch.zeros(n_cols + 1, dtype=torch.int64, device=self.tags.device)
                t_indptr[1:] = torch.cumsum(torch.bincount(tag, minlength=n_cols), 0)
                self._transposed = (t_indptr, ent[order].to(torch.int32).contiguous(), val[order].contiguous())
            return self._transposed
        if self._transposed is None or self._transposed[0].device != self.indptr.device:
            counts = torch.bincount(self.indices.long(), minlength=self.dim)
            t_indptr = torch.zeros(self.dim + 1, dtype=torch.int64, device=self.indptr.device)
            t_indptr[1:] = torch.cumsum(counts, 0)
            row_of = torch.repeat_interleave(torch.arange(self.n_rows, device=self.indptr.device), self.indptr[1:] - self.indptr[:-1])
            order = torch.sort(self.indices.long(), stable=True).indices          # by column, entity rows ascending within one
            t_indices = row_of[order].to(torch.int32).contiguous()
            t_data = None if self.data is None else self.data[order].contiguous()
            self._transposed = (t_indptr, t_indices, t_data)
        return self._transposed


class DeviceCSR(nn.Module):
    """Interaction matrix resident in HBM (non-persistent buffers: they move with ``.to(device)``, stay out of the state_dict).
    ``l2_normalize_rows``: every row is scaled by ``1 / max(||row||_2, 1e-8)`` once, in fp32 (DeepMF's ``normalize_interactions``,
    algorithms/sgd_alg.py:1211-1213, 1226-1228: ``vec / norm.clamp(min=1e-8)`` of the dense row)."""

    def __init__(self, m, l2_normalize_rows: bool = False):
        super().__init__()
        m = sp.csr_matrix(m)
        m.sort_indices()
        self.shape = m.shape
        self.register_buffer('indptr', torch.from_numpy(m.indptr.astype(np.int64)), persistent=False)
        self.register_buffer('indices', torch.from_numpy(m.indices.astype(np.int32)), persistent=False)
        data = torch.from_numpy(m.data.astype(np.float32))
        if l2_normalize_rows:
            counts = torch.from_numpy(np.diff(m.indptr).astype(np.int64))
            row_of = torch.repeat_interleave(torch.arange(m.shape[0]), counts)
            sq = torch.zeros(m.shape[0], dtype=torch.float32).index_add_(0, row_of, data * data)
            data = data / torch.sqrt(sq).clamp(min=1e-8)[row_of]
        self.register_buffer('data', None if bool((data == 1).all()) else data, persistent=False)
        self._transposed = None
        self._t_order = None
        self._grad_ws = None              # [n_rows, C] per-entity gradient rows (ops.SparseLinearActFn, gather form)

    def dense_rows(self, ent: torch.Tensor) -> torch.Tensor:
        """ent: int64 [...] entity ids, -1 = zero vector -> float32 [..., n_cols]."""
        from ._lib import call, ptr, stream
        flat = ent.reshape(-1).long().contiguous()
        out = torch.empty(flat.numel(), self.shape[1], device=flat.device, dtype=torch.float32)
        call('sbr_csr_rows_to_dense', ptr(self.indptr), ptr(self.indices), ptr(self.data), ptr(flat), flat.numel(), self.shape[1],
             ptr(out), out.stride(0), stream())
        return out.view(*ent.shape, self.shape[1])

    def transposed(self):
        """CSR form of the transposed matrix on the matrix's device: (indptr int64 [n_cols + 1], indices int32 [nnz] = rows ascending
        within a column, data float32 [nnz] or None). Built once per device, on first use."""
        if self._transposed is None or self._transposed[0].device != self.indptr.device:
            n_rows, n_cols = self.shape
            dev = self.indptr.device
            cols = self.indices.long()
            t_indptr = torch.zeros(n_cols + 1, dtype=torch.int64, device=dev)
            t_indptr[1:] = torch.cumsum(torch.bincount(cols, minlength=n_cols), 0)
            row_of = torch.repeat_interleave(torch.arange(n_rows, device=dev), self.indptr[1:] - self.indptr[:-1])
            order = torch.sort(cols, stable=True).indices
            self._t_order = order             # entry k of the transposed matrix is entry order[k] of this one (value_view)
            self._transposed = (t_indptr, row_of[order].to(torch.int32).contiguous(),
                                None if self.data is None else self.data[order].contiguous())
        return self._transposed

    def value_view(self) -> 'DeviceCSR':
        """A matrix of the same structure whose values can be replaced (``replace_values``): it shares ``indptr``, ``indices`` and the
        transposed structure with this one, on this one's device, and starts with this one's values (ones for a 0/1 matrix). Mult-VAE's
        input dropout acts on the stored values of the rows; the zeros of a row stay zeros."""
        t_indptr, t_indices, _ = self.transposed()
        v = DeviceCSR.__new__(DeviceCSR)
        nn.Module.__init__(v)
        v.shape = self.shape
        v.register_buffer('indptr', self.indptr, persistent=False)
        v.register_buffer('indices', self.indices, persistent=False)
        v.register_buffer('data', None, persistent=False)
        v._grad_ws = None
        v._t_order = self._t_order
        v._transposed = (t_indptr, t_indices, None)
        return v.replace_values(self.data if self.data is not None else torch.ones(self.indices.numel(), device=self.indices.device))

    def replace_values(self, data: torch.Tensor) -> 'DeviceCSR':
        """(a ``value_view`` only) take ``data``, float32 [nnz] on the matrix's device, as the stored values, in CSR order"""
        if getattr(self, '_t_order', None) is None or self._transposed is None:
            raise RuntimeError('DeviceCSR.replace_values: only a value_view() has replaceable values')
        if data.dtype != torch.float32 or tuple(data.shape) != (self.indices.numel(),) or data.device != self.indices.device:
            raise ValueError(f'DeviceCSR.replace_values: need float32 [{self.indices.numel()}] on {self.indices.device}, got {data.dtype} '
                             f'{tuple(data.shape)} on {data.device}')
        self.data = data
        self._transposed = (self._transposed[0], self._transposed[1], data[self._t_order])
        return self
