"""torch.autograd wrappers around the C-ABI kernels (include/sibrar_hip.h).

PyTorch is used for device memory, streams and the autograd tape only; every forward/backward computation is a HIP
kernel of libsibrar_hip.so. All tensors are fp32 / contiguous CUDA tensors unless stated otherwise. There is no CPU path:
calling any op with CPU tensors raises.
"""
from __future__ import annotations

import numbers
from functools import partial
from typing import List, Optional, Sequence

import torch
from torch.autograd import Function

from ._lib import SibrarHipError, call, lib, ptr, stream

ACT_CODES = {None: 0, 'none': 0, 'relu': 1, 'tanh': 2, 'sigmoid': 3, 'selu': 4}
BN_EPS = 1e-5
BN_MOMENTUM = 0.1
NORM_EPS = 1e-12
PARTITION_MAX_MODALITIES = 8      # sbr_partition_slots (SBR_PART_MAX in rowops.hip)
COLRED_WS_FACTOR = 17             # column-reduction workspaces: totals + SBR_COLRED_REP replicas (colred.h)


# ---- deterministic mode (include/sibrar_hip.h: sbr_set_deterministic; utilities/utils.py:22-27) -----------------------------------
_DET = None                       # cached copy of the library's process-wide flag (None: not read yet)


def is_deterministic() -> bool:
    """True while the library's deterministic mode is on: no kernel of a training step accumulates floats in arrival order, so a
    training repeated from the same parameters, batches, modality draws and dropout seeds gives the same bits."""
    global _DET
    if _DET is None:
        if _os.environ.get('SBR_DETERMINISTIC', '0') == '1':
            set_deterministic(True)
        else:
            _DET = bool(lib().sbr_get_deterministic())
    return _DET


def set_deterministic(flag: bool) -> bool:
    """Switch the deterministic mode (process-wide; returns the previous setting; the env default is ``SBR_DETERMINISTIC=1``).
    Entry points with an arrival-order float accumulation take their fixed-order form, or raise ``SibrarHipError`` ("... no
    deterministic form") where they have none. The captured step graphs of every live ``FusedTrainStep`` are dropped: a captured
    graph has its kernels baked in."""
    global _DET
    prev = bool(lib().sbr_get_deterministic())
    lib().sbr_set_deterministic(1 if flag else 0)
    _DET = bool(flag)
    if prev != _DET:
        from . import engine
        for f in list(engine._LIVE):
            f._graphs.clear()
    return prev


def nondeterministic_launches(reset: bool = False) -> int:
    """Launches of arrival-order float accumulation the library has made since the last reset (counted in both modes)."""
    n = int(lib().sbr_nondeterministic_launches())
    if reset:
        lib().sbr_reset_nondeterministic_launches()
    return n


def act_code(act) -> int:
    if isinstance(act, torch.nn.Module):
        act = act.__class__.__name__.lower()
    if act not in ACT_CODES:
        raise ValueError(f'unsupported activation {act!r}')
    return ACT_CODES[act]


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError('sibrar HIP ops need CUDA(HIP) tensors; there is no CPU fallback in this package')


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


class KernelTimer:
    """Optional HIP-event timing of individual kernel launches on the stream they are launched on (torch's current stream is
    the stream handed to the C ABI). bench.py enables it over plain-launch steps to measure every kernel of the step live:
    ``('call', entry point)`` for every C-ABI call, and the GEMM / scorer wrappers add a key that carries the shape."""
    enabled = False
    records = {}          # key -> [(start_event, stop_event)]

    @classmethod
    def reset(cls, enabled: bool):
        from . import _lib
        cls.enabled, cls.records = enabled, {}
        _lib.CALL_TIMER = cls._bracket if enabled else None

    @classmethod
    def _bracket(cls, name, thunk):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = thunk()
        b.record()
        cls.records.setdefault(('call', name), []).append((a, b))
        key = getattr(_TIMED_KEY, 'value', None)
        if key is not None:              # the shape-carrying key of the wrapper that made this call: the same event pair
            cls.records.setdefault(key, []).append((a, b))
        return rc

    @classmethod
    def results(cls):
        torch.cuda.synchronize()
        return {k: [a.elapsed_time(b) for a, b in v] for k, v in cls.records.items()}


import threading as _threading

_TIMED_KEY = _threading.local()


def _timed(key, fn):
    """``fn`` makes ONE C-ABI call; while KernelTimer is on, the events around that call are also filed under ``key``."""
    if not KernelTimer.enabled:
        return fn()
    _TIMED_KEY.value = key
    try:
        return fn()
    finally:
        _TIMED_KEY.value = None


# ---- raw kernel helpers (no autograd) -------------------------------------------------------------------------------
def gemm(mode: int, A, lda, a_idx, B, ldb, b_idx, bias, C, ldc, c_idx, M, N, K, act=0, atomic=0):
    _timed(('gemm_f32', mode, M, N, K, a_idx is not None or b_idx is not None),
           lambda: call('sbr_gemm_f32', mode, ptr(A), lda, ptr(a_idx), ptr(B), ldb, ptr(b_idx), ptr(bias), ptr(C), ldc,
                        ptr(c_idx), M, N, K, act, atomic, stream()))


import os as _os

_WRES = True                    # weights-resident kernel for N = K = 128 products below the bf16-split kernel's row threshold (tests switch it)
# fp32 products on the bf16 matrix pipe over exact three-way operand splits (csrc/gemm_split_f32.hip); '0' keeps every product on
# the fp32 pipe (v_mfma_f32_32x32x2_f32)
_SPLIT = _os.environ.get('SBR_GEMM_SPLIT', '1') != '0'
_SPLIT_MIN_ROWS = 4096          # below this the per-workgroup weight set-up is not amortised
_WIDE_HEURISTIC = True          # tests switch it off to reach the wide kernel at small shapes


def _mlp_kernel(M, N, K) -> str:
    """Entry point for an N = K = 128 product without gathers (checked by ``_wres_ok``)."""
    if _SPLIT and M >= _SPLIT_MIN_ROWS and lib().sbr_gemm_split_supported(int(M), int(N), int(K)):
        return 'sbr_gemm_split_f32'
    return 'sbr_gemm_wres_f32'


def _wres_ok(M, N, K, *tensors) -> bool:
    """The weights-resident kernel (csrc/gemm_wres_f32.hip) takes the shared MLP's own products: N = K = 128, no gathers,
    16-byte aligned rows."""
    if not _WRES or M < 1 or not lib().sbr_gemm_wres_supported(int(M), int(N), int(K)):
        return False
    return all(t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0 and t.stride(1) == 1 for t in tensors)


def wide_pays(M, N, K) -> bool:
    """Shapes at which the wide bf16-split kernel is used when it could be (measured against the fp32 ring kernel,
    tools/lab/wide_time.py): enough 256 x 256 tiles to fill the chip's 256 workgroup slots, and a wide or deep product (256 x 256
    layers run as fast on the fp32 pipe). bench.py prices a GEMM signature with the same rule."""
    return not _WIDE_HEURISTIC or (-(-M // 256) * (N // 256) >= 176 and max(N, K) >= 512)


def _wide_ok(M, N, K, a, w, out, nt: bool) -> bool:
    """The wide bf16-split kernel (csrc/gemm_split_wide_f32.hip) takes the product: enough rows, N = 256 i, K = 32 j >= 64, 16-byte
    aligned rows of A (and of W for NT), unit column strides."""
    if not _SPLIT or M < _SPLIT_MIN_ROWS or not lib().sbr_gemm_split_wide_supported(int(M), int(N), int(K)):
        return False
    if not wide_pays(M, N, K):
        return False
    ok = a.data_ptr() % 16 == 0 and a.stride(0) % 4 == 0 and a.stride(1) == 1 and w.stride(1) == 1 and out.stride(1) == 1
    return ok and (not nt or (w.data_ptr() % 16 == 0 and w.stride(0) % 4 == 0))


def linear_nt_stats_ok(x, W, out) -> bool:
    """True when ``linear_nt(x, W, ..., out=out, stats_ws=ws)`` can leave the batch statistics of its output pending in ``ws``
    (the bf16-split kernel takes the product: N = K = 128, no gathers, enough rows)."""
    M, (N, K) = x.shape[0], W.shape
    return _wres_ok(M, N, K, x, W, out) and _mlp_kernel(M, N, K) == 'sbr_gemm_split_f32'


def linear_nt(x, W, bias=None, act=0, a_idx=None, out=None, c_idx=None, n_rows=None, stats_ws=None, bn_fin=None):
    """out[ci(m)] = act(x[ai(m)] @ W^T + bias). W: [N, K] with arbitrary row stride (column-major weights are handled by
    the caller through csr kernels, not here). ``stats_ws`` (check ``linear_nt_stats_ok`` first): a zeroed column-reduction
    workspace of 17 * 2 * N doubles that receives the per-column sums and sums of squares of ``out`` (``bn_finalize_stats``).
    ``bn_fin`` (with ``stats_ws``) = (arrive, running_mean, running_var, num_batches_tracked, save_mean, save_rstd, eps, momentum):
    the same launch also finalises the BatchNorm statistics (``arrive``: a zeroed int64[1] owned by the BatchNorm)."""
    M = n_rows if n_rows is not None else (a_idx.numel() if a_idx is not None else x.shape[0])
    N, K = W.shape
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=torch.float32)
    if a_idx is None and c_idx is None and _wres_ok(M, N, K, x, W, out):
        kern = _mlp_kernel(M, N, K)
        if stats_ws is not None and kern != 'sbr_gemm_split_f32':
            raise ValueError('linear_nt(stats_ws=...): this product does not take the kernel with the statistics epilogue')
        if bn_fin is not None:
            if stats_ws is None:
                raise ValueError('linear_nt(bn_fin=...) needs stats_ws')
            arrive, rm, rv, nbt, mean, rstd, eps, mom = bn_fin
            _timed(('gemm_f32', 0, M, N, K, False),
                   lambda: call('sbr_gemm_split_bnstats_f32', ptr(x), x.stride(0), ptr(W), W.stride(0), ptr(bias), ptr(out), out.stride(0),
                                M, N, K, act, ptr(stats_ws), ptr(arrive), ptr(rm), ptr(rv), ptr(nbt), ptr(mean), ptr(rstd), eps, mom,
                                stream()))
            return out
        _timed(('gemm_f32', 0, M, N, K, False),
               lambda: call(kern, 0, ptr(x), x.stride(0), ptr(W), W.stride(0), ptr(bias), ptr(out), out.stride(0), M, N, K,
                            act, None, 0, ptr(stats_ws), stream()))
        return out
    if stats_ws is not None:
        raise ValueError('linear_nt(stats_ws=...): this product does not take the kernel with the statistics epilogue')
    if (_SPLIT and M >= _SPLIT_MIN_ROWS and lib().sbr_gemm_split_proj_supported(int(M), int(N), int(K))
            and all(t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0 and t.stride(1) == 1 for t in (x, W)) and out.stride(1) == 1):
        # dense modality projector (N = 128, K = 768 / 1024 / 2048 ...) on the bf16 matrix pipe, gather and scatter fused
        _timed(('gemm_f32', 0, M, N, K, a_idx is not None),
               lambda: call('sbr_gemm_split_proj_f32', ptr(x), x.stride(0), ptr(a_idx), ptr(W), W.stride(0), ptr(bias), ptr(out),
                            out.stride(0), ptr(c_idx), M, N, K, act, stream()))
        return out
    if _wide_ok(M, N, K, x, W, out, nt=True):
        # wide layers (N = 256 i: hidden widths 256 / 512, the projectors of C = 256 / 512) on the bf16 matrix pipe, gather and scatter fused
        _timed(('gemm_f32', 0, M, N, K, a_idx is not None),
               lambda: call('sbr_gemm_split_wide_f32', 0, ptr(x), x.stride(0), ptr(a_idx), ptr(W), W.stride(0), ptr(bias), ptr(out),
                            out.stride(0), ptr(c_idx), M, N, K, act, stream()))
        return out
    ws_bytes = lib().sbr_gemm_nt_splitk_workspace(M, N, K) if M > 0 else 0
    if ws_bytes > 0:
        # few output tiles, long K (the modality projectors at small batches): K split over workgroups, deterministic reduce
        ws = _tn_workspace(x.device, ws_bytes)
        _timed(('gemm_f32', 0, M, N, K, a_idx is not None),
               lambda: call('sbr_gemm_nt_splitk_f32', ptr(x), x.stride(0), ptr(a_idx), ptr(W), W.stride(0), ptr(bias), ptr(out),
                            out.stride(0), ptr(c_idx), M, N, K, act, ptr(ws), ws.numel() * 4, stream()))
        return out
    gemm(0, x, x.stride(0), a_idx, W, W.stride(0), None, bias, out, out.stride(0), c_idx, M, N, K, act, 0)
    return out


def matmul_nn(dz, W, a_idx=None, n_rows=None, out=None):
    """dz[ai(m)] @ W, W: [K, N] row-major."""
    M = n_rows if n_rows is not None else (a_idx.numel() if a_idx is not None else dz.shape[0])
    K, N = W.shape
    if out is None:
        out = torch.empty(M, N, device=dz.device, dtype=torch.float32)
    if a_idx is None and _wres_ok(M, N, K, dz, W, out):
        _timed(('gemm_f32', 1, M, N, K, False),
               lambda: call(_mlp_kernel(M, N, K), 1, ptr(dz), dz.stride(0), ptr(W), W.stride(0), None, ptr(out), out.stride(0), M, N, K, 0,
                            None, 0, None, stream()))
        return out
    if _wide_ok(M, N, K, dz, W, out, nt=False):
        _timed(('gemm_f32', 1, M, N, K, a_idx is not None),
               lambda: call('sbr_gemm_split_wide_f32', 1, ptr(dz), dz.stride(0), ptr(a_idx), ptr(W), W.stride(0), None, ptr(out),
                            out.stride(0), None, M, N, K, 0, stream()))
        return out
    gemm(1, dz, dz.stride(0), a_idx, W, W.stride(0), None, None, out, out.stride(0), None, M, N, K, 0, 0)
    return out


def matmul_nn_actgrad_ok(dz, W, y, out) -> bool:
    K, N = W.shape
    return _wres_ok(dz.shape[0], N, K, dz, W, y, out)


def matmul_nn_actgrad(dz, W, y, act: int, out, colsum_ws=None):
    """out = (dz @ W) * act'(y) — the gradient at the pre-activation of the layer in front (whose OUTPUT is y) in one kernel;
    ``colsum_ws``: that layer's bias gradient is left pending there (``colred_finish``). Check ``matmul_nn_actgrad_ok`` first."""
    M = dz.shape[0]
    K, N = W.shape
    _timed(('gemm_f32', 1, M, N, K, False),
           lambda: call(_mlp_kernel(M, N, K), 1, ptr(dz), dz.stride(0), ptr(W), W.stride(0), None, ptr(out), out.stride(0), M, N, K, act,
                        ptr(y), y.stride(0), ptr(colsum_ws), stream()))
    return out


_TN_WS = {}
# Workspaces that were outgrown. Their device addresses are baked into every hipGraph captured while they were current
# (engine.FusedTrainStep), so they are never handed back to the caching allocator: a captured step keeps writing its split-K
# slabs into the block it was captured with, and nothing else can be placed there. Growth is geometric, so the retired blocks
# together are smaller than the current one.
_WS_RETIRED = []
WS_GENERATION = 0                 # bumped on every workspace reallocation (tests; diagnostics)


def _grow(table, key, need, make):
    global WS_GENERATION
    old = table.get(key)
    if old is not None:
        _WS_RETIRED.append(old)
        need = max(need, 2 * old.numel())
    table[key] = ws = make(need)
    WS_GENERATION += 1
    return ws


def _device_ws(table, key, n_elems, dtype, floor=0):
    """The grow-only scratch of ``table`` for the device ``key``, with at least ``n_elems`` elements (``floor``: of a first allocation)"""
    ws = table.get(key)
    if ws is None or ws.numel() < n_elems:
        ws = _grow(table, key, max(n_elems, floor), lambda n: torch.empty(n, device=key, dtype=dtype))
    return ws


def _tn_workspace(device, nbytes):
    """Grow-only scratch for the split-K slabs (one per device; reused by every dW product of a step)."""
    return _device_ws(_TN_WS, device, (nbytes + 3) // 4, torch.float32, 1 << 20)


def matmul_tn(dz, x, a_idx=None, b_idx=None, n_rows=None, out=None):
    """sum_r dz[ai(r)]^T x[bi(r)] -> [dz.shape[1], x.shape[1]] (split-K over r with a deterministic slab reducer)."""
    from ._lib import lib
    R = n_rows if n_rows is not None else dz.shape[0]
    M, N = dz.shape[1], x.shape[1]
    if out is None:
        out = torch.empty(M, N, device=dz.device, dtype=torch.float32)
    if R == 0:
        return out.zero_()
    ws_bytes = lib().sbr_gemm_tn_f32_workspace(M, N, R)
    ws = _tn_workspace(dz.device, ws_bytes)
    _timed(('gemm_f32', 2, M, N, R, a_idx is not None or b_idx is not None),
           lambda: call('sbr_gemm_tn_f32', ptr(dz), dz.stride(0), ptr(a_idx), ptr(x), x.stride(0), ptr(b_idx), ptr(out),
                        out.stride(0), M, N, R, ptr(ws), ws.numel() * 4, stream()))
    return out


class DeferredTN:
    """dW products of one backward pass whose split-K slabs are summed by ONE launch at the end (sbr_splitk_reduce_multi).
    Every product keeps its own persistent slab workspace under a caller-chosen key: captured step graphs hold the addresses, so an
    outgrown workspace is retired (kept allocated), never freed. (Measured and dropped: the slab launches themselves as one grouped
    launch at ``finish()`` — 5 us slower per c2 step than one launch per product)"""

    def __init__(self):
        self.ws = {}                 # key -> float32 workspace tensor
        self.pending = []            # (workspace, out, M, N, splits)

    def matmul_tn(self, key, dz, x, a_idx=None, b_idx=None, n_rows=None, out=None):
        import ctypes
        R = n_rows if n_rows is not None else dz.shape[0]
        M, N = dz.shape[1], x.shape[1]
        if R == 0:
            return out.zero_()
        need = lib().sbr_gemm_tn_f32_workspace(M, N, R)
        ws = self.ws.get(key)
        if ws is None or ws.numel() * 4 < need:
            if ws is not None:
                _WS_RETIRED.append(ws)
            ws = self.ws[key] = torch.empty(max((need + 3) // 4, 2 * ws.numel() if ws is not None else 0), device=dz.device,
                                            dtype=torch.float32)
        splits = ctypes.c_int(0)
        _timed(('gemm_f32', 2, M, N, R, a_idx is not None or b_idx is not None),
               lambda: call('sbr_gemm_tn_f32_slabs', ptr(dz), dz.stride(0), ptr(a_idx), ptr(x), x.stride(0), ptr(b_idx), M, N, R,
                            ptr(ws), ws.numel() * 4, ctypes.cast(ctypes.pointer(splits), ctypes.c_void_p), stream()))
        self.pending.append((ws, out, M, N, splits.value))
        return out

    def finish(self, colred=None):
        """Sums the slabs of the pending products. ``colred`` (optional): [(workspace, out float vector [C])] of folded column sums
        — at most 8, with at most 8 pending products — finished by the same launch (``sbr_splitk_reduce_multi_fin``) instead of a
        ``colred_finish`` launch of their own; returns True when they were taken."""
        import ctypes
        took = False
        fuse = colred and 0 < len(colred) <= 8 and 0 < len(self.pending) <= 8
        for lo in range(0, len(self.pending), 8):
            part = self.pending[lo:lo + 8]
            n = len(part)
            arr = lambda ct, vals, m=n: ctypes.cast((ct * m)(*vals), ctypes.c_void_p)
            args = (n, arr(ctypes.c_void_p, [p[0].data_ptr() for p in part]),
                    arr(ctypes.c_void_p, [p[1].data_ptr() for p in part]), arr(ctypes.c_long, [p[1].stride(0) for p in part]),
                    arr(ctypes.c_int, [p[2] for p in part]), arr(ctypes.c_int, [p[3] for p in part]),
                    arr(ctypes.c_int, [p[4] for p in part]))
            # timed as one launch; the key carries every product's (M, N, slabs) so that a reader can apportion it by slab bytes
            key = ('splitk_reduce_multi', tuple((p[2], p[3], p[4]) for p in part))
            if fuse:
                m = len(colred)
                fin = (m, arr(ctypes.c_void_p, [w.data_ptr() for w, _ in colred], m), arr(ctypes.c_void_p, [o.data_ptr() for _, o in colred], m),
                       arr(ctypes.c_int, [o.numel() for _, o in colred], m))
                _timed(key, lambda: call('sbr_splitk_reduce_multi_fin', *args, *fin, stream()))
                took = True
            else:
                _timed(key, lambda: call('sbr_splitk_reduce_multi', *args, stream()))
        self.pending = []
        return took


_COLSUM_WS = {}


def colsum(x: torch.Tensor, out=None) -> torch.Tensor:
    n, C = x.shape
    if out is None:
        out = torch.empty(C, device=x.device, dtype=torch.float32)
    ws = _COLSUM_WS.get((x.device, C))
    if ws is None:
        ws = _COLSUM_WS[(x.device, C)] = torch.zeros(COLRED_WS_FACTOR * C, device=x.device, dtype=torch.float64)
    call('sbr_colsum', ptr(x), x.stride(0), n, C, ptr(out), ptr(ws), stream())
    return out


def act_grad(dy, y, act: int, idx=None, n_rows=None):
    """dz[j] = dy[idx[j]] * act'(y[idx[j]]) (compact [n, C])."""
    n = n_rows if n_rows is not None else (idx.numel() if idx is not None else dy.shape[0])
    C = dy.shape[1]
    dz = torch.empty(n, C, device=dy.device, dtype=torch.float32)
    call('sbr_act_grad_gather', ptr(dy), ptr(y), dy.stride(0), ptr(idx), ptr(dz), C, n, C, act, stream())
    return dz


def colsum_supported(C: int) -> bool:
    """Column sums folded into the producer of their input (sbr_act_grad_gather_colsum, sbr_bn_score_bwd_apply)."""
    return bool(lib().sbr_act_grad_colsum_supported(int(C)))


def new_colsum_ws(device, C: int) -> torch.Tensor:
    """Zeroed column-reduction workspace (totals + replicas) of one pending reduction; its finishing kernel re-zeroes it."""
    return torch.zeros(COLRED_WS_FACTOR * C, device=device, dtype=torch.float64)


def act_grad_colsum(dy, y, act: int, ws, idx=None, n_rows=None):
    """act_grad that also leaves the column sums of its result pending in ``ws`` (complete them with ``colred_finish``)."""
    n = n_rows if n_rows is not None else (idx.numel() if idx is not None else dy.shape[0])
    C = dy.shape[1]
    dz = torch.empty(n, C, device=dy.device, dtype=torch.float32)
    call('sbr_act_grad_gather_colsum', ptr(dy), ptr(y), dy.stride(0), ptr(idx), ptr(dz), C, n, C, act, ptr(ws), stream())
    return dz


def colred_finish(pending) -> None:
    """pending: [(workspace, out float vector [C])] of folded column sums -> one launch per 8 of them."""
    import ctypes
    for lo in range(0, len(pending), 8):
        part = pending[lo:lo + 8]
        n = len(part)
        wsa = (ctypes.c_void_p * n)(*[w.data_ptr() for w, _ in part])
        outa = (ctypes.c_void_p * n)(*[o.data_ptr() for _, o in part])
        ca = (ctypes.c_int * n)(*[o.numel() for _, o in part])
        call('sbr_colred_finish', n, ctypes.cast(wsa, ctypes.c_void_p), ctypes.cast(outa, ctypes.c_void_p),
             ctypes.cast(ca, ctypes.c_void_p), stream())


# ---- Linear (+ activation) ----------------------------------------------------------------------------------------------
class LinearActFn(Function):
    """y = act(x @ W^T + b) — nn.Linear + activation of modules/polylinear.py:51,63-72."""

    @staticmethod
    def forward(ctx, x, weight, bias, act: int):
        _need_cuda(x, weight)
        x = _f32c(x)
        w = weight if weight.stride(1) == 1 else weight.contiguous()
        y = linear_nt(x, w, bias, act)
        ctx.act = act
        ctx.save_for_backward(x, w, y)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        dy = _f32c(dy)
        dz = act_grad(dy, y, ctx.act) if ctx.act else dy
        dx = matmul_nn(dz, w) if ctx.needs_input_grad[0] else None
        dw = matmul_tn(dz, x) if ctx.needs_input_grad[1] else None
        db = colsum(dz) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        return dx, dw, db, None


class SparseLinearActFn(Function):
    """y = act(X[rows] @ W^T + b) with X a resident CSR matrix (``features.DeviceCSR``) that is never densified — the input layer of
    DeepMF's towers (algorithms/sgd_alg.py:1210-1215, 1225-1230: ``dataset.get_*_interaction_vectors(idx).float()`` into
    modules/polylinear.py:51). ``rows``: int32 [n] row ids; ``weight``: [out, n_cols] stored column-major (``weight.t()`` contiguous, the
    layout of FeatureEmbedding's CSR projector); its gradient comes back in the same layout. The weight gradient takes the gather form
    (``sbr_csr_project_bwd_gather``: fixed summation order, no atomics on dW) when ``out % 4 == 0 and out <= 1024``, the scatter form
    otherwise — in deterministic mode the scatter form raises "no deterministic form" instead."""

    @staticmethod
    def forward(ctx, csr, rows, weight, bias, act: int):
        _need_cuda(rows, weight)
        wt = weight.t()
        if not wt.is_contiguous():
            raise ValueError('SparseLinearActFn: the weight must be stored column-major (weight.t() contiguous)')
        if weight.shape[1] != csr.shape[1]:
            raise ValueError(f'SparseLinearActFn: weight has {weight.shape[1]} input columns, the matrix {csr.shape[1]}')
        rows = rows.reshape(-1).to(torch.int32).contiguous()
        n, C = rows.numel(), weight.shape[0]
        y = torch.empty(n, C, device=weight.device, dtype=torch.float32)
        call('sbr_csr_project_fwd', ptr(csr.indptr), ptr(csr.indices), ptr(csr.data), ptr(wt), wt.stride(0), ptr(bias), ptr(rows), ptr(y),
             y.stride(0), None, n, C, act, stream())
        ctx.csr, ctx.act, ctx.has_bias = csr, act, bias is not None
        ctx.save_for_backward(rows, y)
        ctx.w_shape = tuple(weight.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        rows, y = ctx.saved_tensors
        csr = ctx.csr
        C, n_cols = ctx.w_shape
        n = rows.numel()
        dy = _f32c(dy)
        dz = act_grad(dy, y, ctx.act) if ctx.act else dy
        dw = None
        if ctx.needs_input_grad[2]:
            dwt = torch.zeros(n_cols, C, device=dz.device, dtype=torch.float32)
            if C % 4 == 0 and C <= 1024:
                ti, tj, tv = csr.transposed()
                ws = csr._grad_ws
                if ws is None or ws.shape != (csr.shape[0], C) or ws.device != dz.device:
                    ws = csr._grad_ws = torch.empty(csr.shape[0], C, device=dz.device, dtype=torch.float32)
                call('sbr_csr_project_bwd_gather', ptr(ti), ptr(tj), ptr(tv), ptr(dz), dz.stride(0), None, ptr(rows), n, ptr(ws), C,
                     csr.shape[0], ptr(dwt), dwt.stride(0), n_cols, C, stream())
            else:
                # arrival-order float atomics: the library refuses this entry point in deterministic mode ("no deterministic form")
                call('sbr_csr_project_bwd', ptr(csr.indptr), ptr(csr.indices), ptr(csr.data), ptr(dz), dz.stride(0), ptr(rows), ptr(dwt),
                     dwt.stride(0), n, C, stream())
            dw = dwt.t()
        db = colsum(dz) if (ctx.has_bias and ctx.needs_input_grad[3]) else None
        return None, None, dw, db, None


# ---- BatchNorm1d (+ activation) ---------------------------------------------------------------------------------------
class BatchNormActFn(Function):
    """Train-mode BatchNorm1d over rows followed by an activation (polylinear.py:61-65; sgd_alg.py:1837)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, num_batches_tracked, act: int):
        _need_cuda(x, weight)
        x = _f32c(x)
        n, D = x.shape
        y = torch.empty_like(x)
        mean = torch.empty(D, device=x.device, dtype=torch.float32)
        rstd = torch.empty(D, device=x.device, dtype=torch.float32)
        ws = torch.zeros(COLRED_WS_FACTOR * 2 * D, device=x.device, dtype=torch.float64)
        call('sbr_bn_train_fwd', ptr(x), ptr(y), n, D, ptr(weight), ptr(bias), ptr(running_mean), ptr(running_var),
             ptr(num_batches_tracked), ptr(mean), ptr(rstd), ptr(ws), BN_EPS, BN_MOMENTUM, act, stream())
        ctx.act = act
        ctx.save_for_backward(x, y, weight, mean, rstd)
        ctx.mark_non_differentiable(*[t for t in (running_mean, running_var, num_batches_tracked) if t is not None])
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, weight, mean, rstd = ctx.saved_tensors
        dy = _f32c(dy)
        n, D = x.shape
        dx = torch.empty_like(x)
        dw = torch.empty(D, device=x.device, dtype=torch.float32)
        db = torch.empty(D, device=x.device, dtype=torch.float32)
        ws = torch.zeros(COLRED_WS_FACTOR * 2 * D, device=x.device, dtype=torch.float64)
        call('sbr_bn_train_bwd', ptr(dy), ptr(y), ptr(x), ptr(dx), n, D, ptr(weight), ptr(mean), ptr(rstd), ptr(dw), ptr(db),
             ptr(ws), ctx.act, stream())
        return dx, dw, db, None, None, None, None


def batch_norm_eval(x, weight, bias, running_mean, running_var, act: int):
    _need_cuda(x)
    x = _f32c(x)
    y = torch.empty_like(x)
    call('sbr_bn_eval_fwd', ptr(x), ptr(y), x.shape[0], x.shape[1], ptr(weight), ptr(bias), ptr(running_mean),
         ptr(running_var), BN_EPS, act, stream())
    return y


# ---- row normalisation, dropout, aggregation ---------------------------------------------------------------------------
class L2NormalizeFn(Function):
    """F.normalize(x, p=2, dim=-1) — sgd_alg.py:1873-1874. ``eps`` (default ``NORM_EPS``): the clamp of the norm; DeepMF's
    ``x / norm.clamp(min=1e-8)`` (sgd_alg.py:1217-1219) is the same kernel with ``eps=1e-8``."""

    @staticmethod
    def forward(ctx, x, eps: float = NORM_EPS):
        _need_cuda(x)
        x = _f32c(x)
        y = torch.empty_like(x)
        inv = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
        call('sbr_l2norm_fwd', ptr(x), ptr(y), ptr(inv), x.shape[0], x.shape[1], eps, stream())
        ctx.eps = eps
        ctx.save_for_backward(y, inv)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, inv = ctx.saved_tensors
        dy = _f32c(dy)
        dx = torch.empty_like(y)
        call('sbr_l2norm_bwd', ptr(dy), ptr(y), ptr(inv), ptr(dx), y.shape[0], y.shape[1], ctx.eps, stream())
        return dx, None


class DropoutFn(Function):
    """nn.Dropout(p) in training mode with a counter-based mask (seed, element index)."""

    @staticmethod
    def forward(ctx, x, p: float, seed: int):
        _need_cuda(x)
        x = _f32c(x)
        y = torch.empty_like(x)
        call('sbr_dropout', ptr(x), ptr(y), x.numel(), p, seed, stream())
        ctx.p, ctx.seed = p, seed
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _f32c(dy)
        dx = torch.empty_like(dy)
        call('sbr_dropout', ptr(dy), ptr(dx), dy.numel(), ctx.p, ctx.seed, stream())
        return dx, None, None


class AggregateFn(Function):
    """mean / max over the k sampled modalities: [S, k, D] -> [S, D] (sgd_alg.py:27-31, 1861)."""

    @staticmethod
    def forward(ctx, e, mode: int):
        _need_cuda(e)
        e = _f32c(e)
        S, k, D = e.shape
        out = torch.empty(S, D, device=e.device, dtype=torch.float32)
        arg = torch.empty(S, D, device=e.device, dtype=torch.uint8) if mode == 1 else None
        call('sbr_aggregate_fwd', ptr(e), ptr(out), ptr(arg), S, k, D, mode, stream())
        ctx.mode, ctx.shape = mode, (S, k, D)
        ctx.save_for_backward(arg if arg is not None else torch.empty(0, device=e.device))
        return out

    @staticmethod
    def backward(ctx, dout):
        (arg,) = ctx.saved_tensors
        S, k, D = ctx.shape
        dout = _f32c(dout)
        de = torch.empty(S, k, D, device=dout.device, dtype=torch.float32)
        call('sbr_aggregate_bwd', ptr(dout), ptr(arg) if ctx.mode == 1 else None, ptr(de), S, k, D, ctx.mode, stream())
        return de, None


# ---- scorers ----------------------------------------------------------------------------------------------------------------
class ScoreDotFn(Function):
    """einsum('be,bce->bc') — sgd_alg.py:2114."""

    @staticmethod
    def forward(ctx, u, i):
        _need_cuda(u, i)
        u, i = _f32c(u), _f32c(i)
        B, N, D = i.shape
        out = torch.empty(B, N, device=u.device, dtype=torch.float32)
        call('sbr_score_dot_fwd', ptr(u), ptr(i), ptr(out), B, N, D, stream())
        ctx.save_for_backward(u, i)
        return out

    @staticmethod
    def backward(ctx, g):
        u, i = ctx.saved_tensors
        g = _f32c(g)
        B, N, D = i.shape
        du = torch.empty_like(u) if ctx.needs_input_grad[0] else None
        di = torch.empty_like(i) if ctx.needs_input_grad[1] else None
        call('sbr_score_dot_bwd', ptr(g), ptr(u), ptr(i), ptr(du), ptr(di), B, N, D, stream())
        return du, di


COS_EPS = 1e-8                    # nn.CosineSimilarity's default eps (sgd_alg.py:1183)


class ScoreCosFn(Function):
    """nn.CosineSimilarity(dim=-1)(u[:, None, :], i) then ``sim[sim < mu] = mu`` — DeepMF's training scorer, sgd_alg.py:1238-1242:
    u [B, D], i [B, N, D] -> [B, N] in one kernel each way. A floored entry passes no gradient (index assignment cuts the tape)."""

    @staticmethod
    def forward(ctx, u, i, mu: float, eps: float = COS_EPS):
        _need_cuda(u, i)
        u, i = _f32c(u), _f32c(i)
        B, N, D = i.shape
        if u.shape != (B, D):
            raise ValueError(f'ScoreCosFn: u {tuple(u.shape)} does not match i {tuple(i.shape)}')
        out = torch.empty(B, N, device=u.device, dtype=torch.float32)
        raw = torch.empty(B, N, device=u.device, dtype=torch.float32)
        u_stat = torch.empty(B, 2, device=u.device, dtype=torch.float32)
        i_stat = torch.empty(B, N, 2, device=u.device, dtype=torch.float32)
        call('sbr_score_cos_fwd', ptr(u), ptr(i), ptr(out), ptr(raw), ptr(u_stat), ptr(i_stat), B, N, D, mu, eps, stream())
        ctx.mu = mu
        ctx.save_for_backward(u, i, raw, u_stat, i_stat)
        return out

    @staticmethod
    def backward(ctx, g):
        u, i, raw, u_stat, i_stat = ctx.saved_tensors
        g = _f32c(g)
        B, N, D = i.shape
        du = torch.empty_like(u) if ctx.needs_input_grad[0] else None
        di = torch.empty_like(i) if ctx.needs_input_grad[1] else None
        call('sbr_score_cos_bwd', ptr(g), ptr(u), ptr(i), ptr(raw), ptr(u_stat), ptr(i_stat), ptr(du), ptr(di), B, N, D, ctx.mu, stream())
        return du, di, None, None


def floor_scores_(scores: torch.Tensor, mu: float) -> torch.Tensor:
    """In place ``scores[scores < mu] = mu`` (sgd_alg.py:1241) over a 2-D score matrix with unit column stride; NaN stays."""
    _need_cuda(scores)
    if scores.dim() != 2 or scores.dtype != torch.float32 or (scores.shape[1] > 1 and scores.stride(1) != 1):
        raise ValueError('floor_scores_: needs a float32 [n, n_cols] matrix with unit column stride')
    call('sbr_floor_scores', ptr(scores), scores.shape[0], scores.shape[1], scores.stride(0), mu, stream())
    return scores


def l2_normalize_rows(x: torch.Tensor, eps: float = COS_EPS) -> torch.Tensor:
    """x / max(||x||_2, eps) per row, no autograd (the evaluation forms of the cosine scorer)."""
    _need_cuda(x)
    x = _f32c(x)
    y = torch.empty_like(x)
    inv = torch.empty(x.shape[0], device=x.device, dtype=torch.float32)
    call('sbr_l2norm_fwd', ptr(x), ptr(y), ptr(inv), x.shape[0], x.shape[1], eps, stream())
    return y


class ScoreCosAllFn(Function):
    """The all-pairs evaluation form of DeepMF's scorer (sgd_alg.py:1238-1242 on u [Bu, D] x i [I, D], eval/eval.py:216): both sides
    normalised by ``sbr_l2norm_fwd`` (eps 1e-8), the all-pairs GEMM, then the floor — before the caller's exclusion mask, so excluded
    entries stay -inf. Evaluation only: it has no backward."""

    @staticmethod
    def forward(ctx, u, i, mu: float):
        _need_cuda(u, i)
        out = linear_nt(l2_normalize_rows(u), l2_normalize_rows(i))
        ctx.mark_non_differentiable(out)
        return floor_scores_(out, mu)

    @staticmethod
    def backward(ctx, g):
        raise RuntimeError('ScoreCosAllFn is the evaluation form (no_grad); train through ScoreCosFn')


def score_cos_all(u: torch.Tensor, i: torch.Tensor, mu: float) -> torch.Tensor:
    return ScoreCosAllFn.apply(u, i, mu)


class LookupFn(Function):
    """nn.Embedding (dense gradient) — sgd_alg.py:144-145, 159-167: out[..., :] = W[idx[...], :]; dW is the dense scatter-add."""

    @staticmethod
    def forward(ctx, W, idx):
        _need_cuda(W, idx)
        if W.stride(-1) != 1:
            W = W.contiguous()
        rows = idx.reshape(-1).to(torch.int32).contiguous()
        n, D = rows.numel(), W.shape[1]
        out = torch.empty(n, D, device=W.device, dtype=torch.float32)
        call('sbr_gather_rows', ptr(W), W.stride(0), ptr(rows), ptr(out), D, None, n, D, stream())
        ctx.save_for_backward(rows)
        ctx.w_shape = W.shape
        return out.view(*idx.shape, D)

    @staticmethod
    def backward(ctx, g):
        (rows,) = ctx.saved_tensors
        D = ctx.w_shape[1]
        g = _f32c(g).reshape(-1, D)
        dW = torch.zeros(ctx.w_shape, device=g.device, dtype=torch.float32)
        call('sbr_scatter_add_rows', ptr(g), D, None, ptr(rows), ptr(dW), D, rows.numel(), D, stream())
        return dW, None


class GatherLinearFn(Function):
    """nn.Linear(bias=False) on looked-up rows — UIProtoMF's projections, sgd_alg.py:575, 581: ``table[idx] @ weight^T`` with the
    gather fused into the GEMM; the table gradient is the dense scatter-add of ``LookupFn``."""

    @staticmethod
    def forward(ctx, table, idx, weight):
        _need_cuda(table, idx, weight)
        if table.stride(-1) != 1:
            table = table.contiguous()
        w = weight if weight.stride(1) == 1 else weight.contiguous()
        rows = idx.reshape(-1).to(torch.int32).contiguous()
        out = linear_nt(table, w, a_idx=rows)
        ctx.save_for_backward(table, rows, w)
        return out.view(*idx.shape, w.shape[0])

    @staticmethod
    def backward(ctx, g):
        table, rows, w = ctx.saved_tensors
        n, D = rows.numel(), table.shape[1]
        g = _f32c(g).reshape(n, w.shape[0])
        d_table = None
        if ctx.needs_input_grad[0]:
            dx = matmul_nn(g, w)
            d_table = torch.zeros(table.shape, device=g.device, dtype=torch.float32)
            call('sbr_scatter_add_rows', ptr(dx), D, None, ptr(rows), ptr(d_table), D, n, D, stream())
        dw = matmul_tn(g, table, b_idx=rows) if ctx.needs_input_grad[2] else None
        return d_table, None, dw


# ---- the three fused model ops on the 64 x 64 fp32 tile skeleton (csrc/tile64_f32.h): shared operand checks, workspaces, table gradient ----
def _tile_operands(table, idx, matrix, who, noun, count, max_d, max_n):
    """``table[idx]`` against the rows of ``matrix`` (``noun``: 'prototypes' / 'anchors', counted as ``count``): shape and range errors
    are ``ValueError`` before anything touches the device. -> (table, rows, matrix, R, D, N)"""
    if table.dim() != 2 or matrix.dim() != 2 or table.shape[1] != matrix.shape[1]:
        raise ValueError(f'{who}: table {tuple(table.shape)} and {noun} {tuple(matrix.shape)} must be matrices of one width')
    D, N = int(table.shape[1]), int(matrix.shape[0])
    if not (1 <= D <= max_d and 2 <= N <= max_n):
        raise ValueError(f'{who}: needs 1 <= embedding_dim <= {max_d} and 2 <= {count} <= {max_n}, got {D} and {N}')
    _need_cuda(table, idx, matrix)
    table = _f32c(table) if table.stride(-1) != 1 or table.dtype != torch.float32 else table
    rows = None if idx is None else idx.reshape(-1).to(torch.int32).contiguous()
    R = table.shape[0] if rows is None else rows.numel()
    return table, rows, _f32c(matrix), R, D, N


def _tile_ws(entry, device, R, D, N, backward, min_bytes=8):
    """the workspace that ``entry`` (a ``*_workspace`` entry point) asks for, never empty"""
    n = int(getattr(lib(), entry)(R, D, N, 1 if backward else 0))
    return torch.empty(max(n, min_bytes), device=device, dtype=torch.uint8)


def _tile_view(out, idx):
    """out [R, n] as [*idx.shape, n] (``idx`` None: the rows are the table's)"""
    return out if idx is None else out.view(*idx.shape, out.shape[1])


def _tile_grads(entry, device, R, D, N, need_t, need_n):
    """the outputs of a backward entry point, each where needed: dE [R, D], the [N, D] gradient of the matrix, and ``entry``'s backward
    workspace (the matrix gradient's). -> (dE, dN, ws, ws bytes)"""
    dE = torch.empty(R, D, device=device, dtype=torch.float32) if need_t else None
    dN = torch.empty(N, D, device=device, dtype=torch.float32) if need_n else None
    ws = _tile_ws(entry, device, R, D, N, True) if need_n and R > 0 else None
    return dE, dN, ws, 0 if ws is None else ws.numel()


def _table_grad(table, rows, dE):
    """the dense table gradient from dE [R, D] = d / d table[rows] (``rows`` None: the rows are the table), as ``LookupFn`` returns it;
    None where dE is None (the table needs no gradient)"""
    if dE is None:
        return None
    d_table = torch.zeros(table.shape, device=dE.device, dtype=torch.float32)
    if rows is None:
        d_table.copy_(dE)
    elif rows.numel() > 0:
        D = table.shape[1]
        call('sbr_scatter_add_rows', ptr(dE), D, None, ptr(rows), ptr(d_table), D, rows.numel(), D, stream())
    return d_table


# ---- ProtoMF: shifted cosine similarity to the prototypes -----------------------------------------------------------------------------
PROTO_MAX_D, PROTO_MAX_P = 512, 256          # csrc/proto_cos.hip


def _proto_operands(table, idx, prototypes, who):
    return _tile_operands(table, idx, prototypes, who, 'prototypes', 'n_prototypes', PROTO_MAX_D, PROTO_MAX_P)


def _proto_sim_fwd(table, rows, protos, R, D, P, cos=None, saved=(None,) * 7):
    """``sbr_proto_sim_fwd`` -> sim [R, P]. ``cos``: where the un-clamped cosine goes; ``saved``: row_stat, proto_stat, row_best, col_val,
    col_row, proto_loss, batch_loss of the training form"""
    sim = torch.empty(R, P, device=table.device, dtype=torch.float32)
    ws = _tile_ws('sbr_proto_sim_workspace', table.device, R, D, P, False)
    _timed(('proto_sim_fwd', R, D, P),
           lambda: call('sbr_proto_sim_fwd', ptr(table), table.stride(0), ptr(rows), R, D, ptr(protos), P, ptr(sim), ptr(cos),
                        *map(ptr, saved), ptr(ws), ws.numel(), stream()))
    return sim


class ProtoSimFn(Function):
    """ProtoMF's prototype side in one op — sgd_alg.py:48-59 (compute_shifted_cosine_sim) on ``table[idx]`` against ``prototypes``
    (sgd_alg.py:381-382, 486-488) plus the two regularisers of compute_reg_losses (sgd_alg.py:394-399, 505-510):
    ``-> (sim [*idx.shape, P], proto_loss, batch_loss)`` with proto_loss = mean_p min_j (2 - sim), batch_loss = mean_j min_p (2 - sim) as
    device scalars. The lookup is fused (no gathered or normalised copy is written); the backward pass routes the arg-min gradients
    inside the kernel (ties: the lowest index) and returns the dense table gradient, as ``LookupFn`` does. One fixed-order form."""

    @staticmethod
    def forward(ctx, table, idx, prototypes):
        table, rows, protos, R, D, P = _proto_operands(table, idx, prototypes, 'ProtoSimFn')
        dev = table.device
        f32 = dict(device=dev, dtype=torch.float32)
        cos = torch.empty(R, P, **f32)
        row_stat, proto_stat = torch.empty(R, 2, **f32), torch.empty(P, 2, **f32)
        row_best = torch.empty(R, device=dev, dtype=torch.int32)
        col_val, col_row = torch.empty(P, **f32), torch.empty(P, device=dev, dtype=torch.int32)
        proto_loss, batch_loss = torch.zeros((), **f32), torch.zeros((), **f32)
        sim = _proto_sim_fwd(table, rows, protos, R, D, P, cos, (row_stat, proto_stat, row_best, col_val, col_row, proto_loss, batch_loss))
        ctx.save_for_backward(table, rows, protos, cos, row_stat, proto_stat, row_best, col_row)
        return _tile_view(sim, idx), proto_loss, batch_loss

    @staticmethod
    def backward(ctx, g_sim, g_proto, g_batch):
        table, rows, protos, cos, row_stat, proto_stat, row_best, col_row = ctx.saved_tensors
        (R, P), D = cos.shape, table.shape[1]
        g_sim = _f32c(g_sim).reshape(R, P)
        g_proto, g_batch = (None if g is None else g.reshape(1).float().contiguous() for g in (g_proto, g_batch))
        dE, dP, ws, ws_bytes = _tile_grads('sbr_proto_sim_workspace', cos.device, R, D, P, ctx.needs_input_grad[0], ctx.needs_input_grad[2])
        _timed(('proto_sim_bwd', R, D, P),
               lambda: call('sbr_proto_sim_bwd', ptr(g_sim), ptr(g_proto), ptr(g_batch), ptr(table), table.stride(0), ptr(rows), R, D,
                            ptr(protos), P, ptr(cos), ptr(row_stat), ptr(proto_stat), ptr(row_best), ptr(col_row), ptr(dE), ptr(dP),
                            ptr(ws), ws_bytes, stream()))
        return _table_grad(table, rows, dE), None, dP


def proto_sim(table: torch.Tensor, idx: Optional[torch.Tensor], prototypes: torch.Tensor) -> torch.Tensor:
    """The evaluation form of ``ProtoSimFn`` (no autograd, no arg-mins): clamp(1 + cos(table[idx], prototypes), 0, 2) as
    [*idx.shape, P]; ``idx`` None: every row of ``table``."""
    table, rows, protos, R, D, P = _proto_operands(table.detach(), idx, prototypes.detach(), 'proto_sim')
    return _tile_view(_proto_sim_fwd(table, rows, protos, R, D, P), idx)


def cosine_sim(table: torch.Tensor, idx: Optional[torch.Tensor], others: torch.Tensor) -> torch.Tensor:
    """sgd_alg.py:62-73 (compute_cosine_sim): clamp(cos(table[idx], others), -1, 1) as [*idx.shape, P] — the un-clamped cosine that
    ``sbr_proto_sim_fwd`` writes next to the shifted similarity, clamped in place. No autograd (ACF's post_val statistics)."""
    table, rows, others, R, D, P = _proto_operands(table.detach(), idx, others.detach(), 'cosine_sim')
    cos = torch.empty(R, P, device=table.device, dtype=torch.float32)
    _proto_sim_fwd(table, rows, others, R, D, P, cos)
    return _tile_view(cos.clamp_(min=-1., max=1.), idx)


# ---- ProtoMFs: plain cosine similarity to the prototypes, and its dot with the relu'd weights of the other entity -------------------------
class ProtoCosFn(Function):
    """sgd_alg.py:62-73 (compute_cosine_sim) on ``table[idx]`` against ``prototypes`` (sgd_alg.py:677-678, 742-746), differentiable:
    ``-> clamp(cos, -1, 1) [*idx.shape, P]`` (``idx`` None: every row of ``table``). The lookup is fused; the backward pass returns the
    dense table gradient, as ``LookupFn`` does, and the prototype gradient. One fixed-order form (csrc/proto_cos.hip)."""

    @staticmethod
    def forward(ctx, table, idx, prototypes):
        table, rows, protos, R, D, P = _proto_operands(table, idx, prototypes, 'ProtoCosFn')
        f32 = dict(device=table.device, dtype=torch.float32)
        cos, raw = torch.empty(R, P, **f32), torch.empty(R, P, **f32)
        row_stat, proto_stat = torch.empty(R, 2, **f32), torch.empty(P, 2, **f32)
        ws = _tile_ws('sbr_proto_score_workspace', table.device, R, D, P, False)
        _timed(('proto_score_fwd', R, D, P, 0),
               lambda: call('sbr_proto_score_fwd', ptr(table), table.stride(0), ptr(rows), R, D, ptr(protos), P, None, 0, None, 1, ptr(cos),
                            None, ptr(raw), ptr(row_stat), ptr(proto_stat), ptr(ws), ws.numel(), stream()))
        ctx.save_for_backward(table, rows, protos, raw, row_stat, proto_stat)
        return _tile_view(cos, idx)

    @staticmethod
    def backward(ctx, g):
        table, rows, protos, raw, row_stat, proto_stat = ctx.saved_tensors
        (R, P), D = raw.shape, table.shape[1]
        g = _f32c(g).reshape(R, P)
        dE, dP, ws, ws_bytes = _tile_grads('sbr_proto_score_workspace', raw.device, R, D, P, ctx.needs_input_grad[0], ctx.needs_input_grad[2])
        _timed(('proto_score_bwd', R, D, P, 0),
               lambda: call('sbr_proto_score_bwd', ptr(g), ptr(table), table.stride(0), ptr(rows), R, D, ptr(protos), P, None, 0, None, 1,
                            ptr(raw), ptr(row_stat), ptr(proto_stat), ptr(dE), ptr(dP), None, ptr(ws), ws_bytes, stream()))
        return _table_grad(table, rows, dE), None, dP


class ProtoScoreFn(Function):
    """The training logit of the simplified ProtoMF family in one op — sgd_alg.py:676-688, 738-751, 806-826:
    ``out[j, f] = sum_p clamp(cos(table[idx[j]], prototypes[p]), -1, 1) * relu(weights[widx[j * fan + f], p]) -> [R, fan]``, R =
    idx.numel(). ``widx`` None: ``weights`` holds the R * fan weight rows themselves, in order. Neither the cosines' lookup nor the
    relu'd weight gather is written. The backward pass returns the dense table gradient, the prototype gradient and the weight
    gradient: dense (scattered over ``widx``) when ``widx`` is given, the row gradient itself when it is None; zero where
    ``weights <= 0``, as torch's ReLU. One fixed-order form (csrc/proto_cos.hip)."""

    @staticmethod
    def forward(ctx, table, idx, prototypes, weights, widx, fan):
        fan = int(fan)
        if weights.dim() != 2 or prototypes.dim() != 2 or weights.shape[1] != prototypes.shape[0]:
            raise ValueError(f'ProtoScoreFn: weights {tuple(weights.shape)} must be a matrix as wide as the n_prototypes of prototypes '
                             f'{tuple(prototypes.shape)}')
        R = int(table.shape[0] if idx is None else idx.numel()) if table.dim() == 2 else 0
        n_w = int(weights.shape[0] if widx is None else widx.numel())
        if fan < 1 or n_w != R * fan or R * fan >= 2 ** 31:
            raise ValueError(f'ProtoScoreFn: needs 1 <= fan, R * fan < 2^31 and R * fan weight rows ({"weights" if widx is None else "widx"}), '
                             f'got R = {R}, fan = {fan} and {n_w}')
        table, rows, protos, R, D, P = _proto_operands(table, idx, prototypes, 'ProtoScoreFn')
        _need_cuda(weights, widx)
        wt = _f32c(weights) if weights.stride(-1) != 1 or weights.dtype != torch.float32 else weights
        wrows = None if widx is None else widx.reshape(-1).to(torch.int32).contiguous()
        f32 = dict(device=table.device, dtype=torch.float32)
        out, raw = torch.empty(R, fan, **f32), torch.empty(R, P, **f32)
        row_stat, proto_stat = torch.empty(R, 2, **f32), torch.empty(P, 2, **f32)
        ws = _tile_ws('sbr_proto_score_workspace', table.device, R, D, P, False)
        _timed(('proto_score_fwd', R, D, P, fan),
               lambda: call('sbr_proto_score_fwd', ptr(table), table.stride(0), ptr(rows), R, D, ptr(protos), P, ptr(wt), wt.stride(0),
                            ptr(wrows), fan, None, ptr(out), ptr(raw), ptr(row_stat), ptr(proto_stat), ptr(ws), ws.numel(), stream()))
        ctx.save_for_backward(table, rows, protos, wt, wrows, raw, row_stat, proto_stat)
        ctx.fan = fan
        return out

    @staticmethod
    def backward(ctx, g):
        table, rows, protos, wt, wrows, raw, row_stat, proto_stat = ctx.saved_tensors
        (R, P), D, fan = raw.shape, table.shape[1], ctx.fan
        g = _f32c(g).reshape(R, fan)
        dE, dP, ws, ws_bytes = _tile_grads('sbr_proto_score_workspace', raw.device, R, D, P, ctx.needs_input_grad[0], ctx.needs_input_grad[2])
        dW = torch.empty(R * fan, P, device=raw.device, dtype=torch.float32) if ctx.needs_input_grad[3] else None
        _timed(('proto_score_bwd', R, D, P, fan),
               lambda: call('sbr_proto_score_bwd', ptr(g), ptr(table), table.stride(0), ptr(rows), R, D, ptr(protos), P, ptr(wt),
                            wt.stride(0), ptr(wrows), fan, ptr(raw), ptr(row_stat), ptr(proto_stat), ptr(dE), ptr(dP), ptr(dW), ptr(ws),
                            ws_bytes, stream()))
        if wrows is not None:
            dW = _table_grad(wt, wrows, dW)
        return _table_grad(table, rows, dE), None, dP, dW, None, None


# ---- ACF: softmax mixing of the anchors ------------------------------------------------------------------------------------------------
ANCHOR_MAX_D, ANCHOR_MAX_K = 512, 256        # csrc/anchor_mix.hip
ANCHOR_TILE, ANCHOR_MAX_WG = 64, 1024        # rows of a workgroup's tile, grid cap of either pass (AM_T, AM_MAX_WG)


def _anchor_operands(table, idx, anchors, who):
    return _tile_operands(table, idx, anchors, who, 'anchors', 'n_anchors', ANCHOR_MAX_D, ANCHOR_MAX_K)


class AnchorMixFn(Function):
    """One side of ACF in one op — sgd_alg.py:261-276 on ``table[idx]`` against ``anchors`` plus, with ``with_losses``, the two entropy
    regularisers of ACF.forward (sgd_alg.py:246-254): ``-> (r [*idx.shape, D], c [*idx.shape, K], exc_loss, inc_loss)`` with
    c = softmax(table[idx] @ anchors^T), r = c @ anchors, exc_loss = mean entropy_from_softmax(c, logits), inc_loss = log K - H(q) as
    device scalars (zeros without ``with_losses``). ``c`` is marked NON-DIFFERENTIABLE: gradients flow through ``r`` and the two losses
    only, which is every use the model makes of it. The lookup is fused and the logits are never written; the backward pass recomputes
    them and returns the dense table gradient, as ``LookupFn`` does. A column of ``c`` that is zero in every row makes ``inc_loss``
    NaN, as in the reference. One fixed-order form (valid in deterministic mode)."""

    @staticmethod
    def forward(ctx, table, idx, anchors, with_losses: bool):
        table, rows, anc, R, D, K = _anchor_operands(table, idx, anchors, 'AnchorMixFn')
        dev = table.device
        f32 = dict(device=dev, dtype=torch.float32)
        r, c, lse = torch.empty(R, D, **f32), torch.empty(R, K, **f32), torch.empty(R, **f32)
        exc, inc = torch.zeros((), **f32), torch.zeros((), **f32)
        q = dinc = ws = None
        if with_losses and R > 0:
            q, dinc = torch.empty(K, **f32), torch.empty(K, **f32)
            ws = _tile_ws('sbr_anchor_mix_workspace', dev, R, D, K, False)
        if R > 0:
            _timed(('anchor_mix_fwd', R, D, K),
                   lambda: call('sbr_anchor_mix_fwd', ptr(table), table.stride(0), ptr(rows), R, D, ptr(anc), K, ptr(r), ptr(c), ptr(lse),
                                ptr(q), ptr(dinc), ptr(exc) if q is not None else None, ptr(inc) if q is not None else None, ptr(ws),
                                0 if ws is None else ws.numel(), stream()))
        ctx.save_for_backward(table, rows, anc, c, lse, dinc)
        ctx.with_losses = q is not None
        c_out = _tile_view(c, idx)
        ctx.mark_non_differentiable(c_out)
        return _tile_view(r, idx), c_out, exc, inc

    @staticmethod
    def backward(ctx, g_r, _g_c, g_exc, g_inc):
        table, rows, anc, c, lse, dinc = ctx.saved_tensors
        (R, K), D = c.shape, table.shape[1]
        g_r = _f32c(g_r).reshape(R, D)
        if not ctx.with_losses:
            g_exc = g_inc = None
        g_exc, g_inc = (None if g is None else g.reshape(1).float().contiguous() for g in (g_exc, g_inc))
        dE, dA, ws, ws_bytes = _tile_grads('sbr_anchor_mix_workspace', c.device, R, D, K, ctx.needs_input_grad[0], ctx.needs_input_grad[2])
        _timed(('anchor_mix_bwd', R, D, K),
               lambda: call('sbr_anchor_mix_bwd', ptr(g_r), ptr(g_exc), ptr(g_inc), ptr(table), table.stride(0), ptr(rows), R, D, ptr(anc),
                            K, ptr(c), ptr(lse), ptr(dinc), ptr(dE), ptr(dA), ptr(ws), ws_bytes, stream()))
        return _table_grad(table, rows, dE), None, dA, None


def anchor_mix(table: torch.Tensor, idx: Optional[torch.Tensor], anchors: torch.Tensor, want: str = 'r') -> torch.Tensor:
    """The evaluation form of ``AnchorMixFn`` (no autograd, no losses): ``want='r'`` -> softmax(table[idx] @ anchors^T) @ anchors as
    [*idx.shape, D]; ``want='c'`` -> the softmax itself as [*idx.shape, K]. ``idx`` None: every row of ``table``."""
    if want not in ('r', 'c'):
        raise ValueError(f"anchor_mix: want must be 'r' or 'c', got {want!r}")
    table, rows, anc, R, D, K = _anchor_operands(table.detach(), idx, anchors.detach(), 'anchor_mix')
    n = D if want == 'r' else K
    out = torch.empty(R, n, device=table.device, dtype=torch.float32)
    if R > 0:
        _timed(('anchor_mix_fwd', R, D, K),
               lambda: call('sbr_anchor_mix_fwd', ptr(table), table.stride(0), ptr(rows), R, D, ptr(anc), K, ptr(out) if want == 'r' else None,
                            ptr(out) if want == 'c' else None, None, None, None, None, None, None, 0, stream()))
    return _tile_view(out, idx)


# ---- ECF: sparse affiliation of a row to its clusters ----------------------------------------------------------------------------------
CLUSTER_MAX_D, CLUSTER_MAX_C = 512, 256      # csrc/cluster_affil.hip
CLUSTER_TILE = 64                            # rows of a workgroup's tile (CA_T)


def _cluster_operands(table, clusters, logits, top, temp, who):
    """The operand checks of either form (``logits`` None: the cosine form on ``table`` x ``clusters``; otherwise the logit form):
    shape and range errors are ``ValueError`` before anything touches the device."""
    cosine = logits is None
    if cosine:
        if table is None or clusters is None or table.dim() != 2 or clusters.dim() != 2 or table.shape[1] != clusters.shape[1]:
            raise ValueError(f'{who}: the cosine form needs a table and clusters that are matrices of one width')
        D, C = int(table.shape[1]), int(clusters.shape[0])
        if not 1 <= D <= CLUSTER_MAX_D:
            raise ValueError(f'{who}: needs 1 <= embedding_dim <= {CLUSTER_MAX_D}, got {D}')
    else:
        if table is not None or clusters is not None:
            raise ValueError(f'{who}: the logit form takes the logits alone')
        if logits.dim() != 2:
            raise ValueError(f'{who}: the logits {tuple(logits.shape)} must be a matrix [rows, n_clusters]')
        D, C = 0, int(logits.shape[1])
    if not 2 <= C <= CLUSTER_MAX_C:
        raise ValueError(f'{who}: needs 2 <= n_clusters <= {CLUSTER_MAX_C}, got {C}')
    if not (isinstance(top, numbers.Integral) and 1 <= int(top) <= C):
        raise ValueError(f'{who}: needs an integer 1 <= top <= n_clusters = {C}, got {top!r}')
    if not float(temp) > 0:
        raise ValueError(f'{who}: needs temp > 0, got {temp!r}')
    _need_cuda(table, clusters, logits)
    if cosine:
        table = _f32c(table) if table.stride(-1) != 1 or table.dtype != torch.float32 else table
        return table, _f32c(clusters), None, int(table.shape[0]), D, C
    logits = _f32c(logits)
    return None, None, logits, int(logits.shape[0]), D, C


def _cluster_fwd(table, clusters, logits, R, D, C, top, temp, want_state):
    dev = (table if logits is None else logits).device
    f32 = dict(device=dev, dtype=torch.float32)
    t = torch.empty(R, C, **f32) if logits is None else None
    x = torch.empty(R, C, **f32)
    state = torch.empty(R, 4, **f32) if want_state else None
    mask = torch.empty(R, (C + 3) // 4, device=dev, dtype=torch.uint8) if want_state else None
    if R > 0:
        ws = _tile_ws('sbr_cluster_affil_workspace', dev, R, D, C, False, 16) if logits is None else None
        _timed(('cluster_affil_fwd', R, D, C),
               lambda: call('sbr_cluster_affil_fwd', ptr(table), 0 if table is None else table.stride(0), ptr(clusters), ptr(logits), R, D, C,
                            int(top), float(temp), ptr(t), ptr(x), ptr(state), ptr(mask), ptr(ws), 0 if ws is None else ws.numel(), stream()))
    return t, x, state, mask


class ClusterAffilFn(Function):
    """ECF's affiliation of a row to its ``top`` clusters in one op each way (csrc/cluster_affil.hip) — sgd_alg.py:1020-1037 and
    988-1009: ``x = sigmoid(t) * (p + (m - p).detach())`` with m the exact top-``top`` mask of a row of t and p = softmax(t / temp).

    Cosine form ``apply(table, clusters, None, top, temp) -> (t, x)``: the rows are the WHOLE table, t = clamp(cos(table, clusters), -1, 1)
    [R, C]. ``t`` is a differentiable output: a gradient into it (ECF's user side reads the item logits) is added inside the backward
    kernel. The table gradient is dense and written directly. Logit form ``apply(None, None, logits, top, temp) -> x``.
    Equal logits at the mask boundary go to the lowest cluster index. One fixed-order form (valid in deterministic mode)."""

    @staticmethod
    def forward(ctx, table, clusters, logits, top, temp):
        table, cl, lg, R, D, C = _cluster_operands(table, clusters, logits, top, temp, 'ClusterAffilFn')
        t, x, state, mask = _cluster_fwd(table, cl, lg, R, D, C, top, temp, True)
        ctx.cosine, ctx.temp, ctx.dims = lg is None, float(temp), (R, D, C)
        ctx.set_materialize_grads(False)
        if lg is None:
            ctx.save_for_backward(table, cl, t, state, mask)
            return t, x
        ctx.save_for_backward(lg, state, mask)
        return x

    @staticmethod
    def backward(ctx, *grads):
        R, D, C = ctx.dims
        if ctx.cosine:
            table, cl, t, state, mask = ctx.saved_tensors
            g_t, g_x = grads
            dev = t.device
            need_w, need_c = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
            g_x = torch.zeros(R, C, device=dev, dtype=torch.float32) if g_x is None else _f32c(g_x)
            g_t = None if g_t is None else _f32c(g_t)
            dW = torch.empty(R, D, device=dev, dtype=torch.float32) if need_w else None
            if R == 0:                       # no rows: nothing to launch (an empty table has no device pointer either)
                return dW, torch.zeros(C, D, device=dev, dtype=torch.float32) if need_c else None, None, None, None
            dC = torch.empty(C, D, device=dev, dtype=torch.float32) if need_c else None
            ws = _tile_ws('sbr_cluster_affil_workspace', dev, R, D, C, True, 16) if need_w or need_c else None
            _timed(('cluster_affil_bwd', R, D, C),
                   lambda: call('sbr_cluster_affil_bwd', ptr(g_x), ptr(g_t), ptr(table), table.stride(0), ptr(cl), ptr(t), R, D, C, ctx.temp,
                                ptr(state), ptr(mask), ptr(dW), D, ptr(dC), None, ptr(ws), 0 if ws is None else ws.numel(), stream()))
            return dW, dC, None, None, None
        lg, state, mask = ctx.saved_tensors
        (g_x,) = grads
        d = None
        if ctx.needs_input_grad[2]:
            g_x = torch.zeros(R, C, device=lg.device, dtype=torch.float32) if g_x is None else _f32c(g_x)
            d = torch.empty(R, C, device=lg.device, dtype=torch.float32)
            if R > 0:
                _timed(('cluster_affil_bwd', R, 0, C),
                       lambda: call('sbr_cluster_affil_bwd', ptr(g_x), None, None, 0, None, ptr(lg), R, 0, C, ctx.temp, ptr(state), ptr(mask),
                                    None, 0, None, ptr(d), None, 0, stream()))
        return None, None, d, None, None


def cluster_affil(table, clusters, logits, top: int, temp: float):
    """The evaluation form of ``ClusterAffilFn`` (no autograd, nothing saved): ``(t, x)`` in the cosine form, ``x`` in the logit form."""
    table, cl, lg, R, D, C = _cluster_operands(None if table is None else table.detach(), None if clusters is None else clusters.detach(),
                                               None if logits is None else logits.detach(), top, temp, 'cluster_affil')
    t, x, _, _ = _cluster_fwd(table, cl, lg, R, D, C, top, temp, False)
    return (t, x) if lg is None else x


def csr_rows_times_dense(csr, rows: torch.Tensor, dense: torch.Tensor) -> torch.Tensor:
    """``X[rows] @ dense`` with X a resident ``features.DeviceCSR`` [n, n_cols] and ``dense`` [n_cols, C] contiguous — ECF's
    ``Y[u_idxs] @ x_tildes`` (sgd_alg.py:992) and ``tag_matrix^T @ xs`` (sgd_alg.py:957, transposed). ``SparseLinearActFn`` with the dense
    operand as its column-major weight: the gradient of ``dense`` takes the gather form (fixed order) when ``C % 4 == 0``, the scatter
    form otherwise, which deterministic mode refuses ("no deterministic form")."""
    if dense.dim() != 2 or not dense.is_contiguous():
        raise ValueError('csr_rows_times_dense: the dense operand must be a contiguous matrix [n_cols, C]')
    return SparseLinearActFn.apply(csr, rows, dense.t(), None, 0)


# ---- operands of the fit-matrix entries (knn.hip, ease.hip, p3alpha.hip, als.hip, svd.hip, rbmf.hip) --------------------------------------
BLOCK_MAX = 128                   # columns of a dense block: ALS factors, the SVD's block, RBMF's representatives (csrc/block128.h)
SVD_MAX_BLOCK = MAXVOL_MAX_R = BLOCK_MAX


def _block_width(who, c, n=None):
    """Refuses a dense block of ``c`` columns outside [1, BLOCK_MAX] and (``n`` given) one of fewer rows than columns"""
    if not 1 <= c <= BLOCK_MAX or (n is not None and n < c):
        raise ValueError(f'{who}: {c} columns, outside [1, {BLOCK_MAX}]' + ('' if n is None else f', or more than its {n} rows'))


def _row_range(rows, n, who=None):
    """``(r0, r1, whole)`` of ``rows=(r0, r1)`` among ``n`` rows (None: every row). ``who``: the caller's name, to refuse a range outside
    [0, n] here (None: the C entry refuses it)"""
    r0, r1 = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
    if who is not None and not 0 <= r0 <= r1 <= n:
        raise ValueError(f'{who}: row range [{r0}, {r1}) outside [0, {n}]')
    return r0, r1, (r0, r1) == (0, n)


_ENTRY_WS = {}                    # entry -> device -> its scratch


def _entry_ws(device, entry, *args, dtype=torch.float32):
    """``(pointer, bytes)`` of ``entry``'s grow-only scratch on ``device`` (elements of ``dtype``), grown to what the library's
    ``<entry>_workspace(*args)`` asks for; ``(None, 0)`` when it asks for nothing"""
    need = int(getattr(lib(), entry + '_workspace')(*args))
    if need == 0:
        return None, 0
    ws = _device_ws(_ENTRY_WS.setdefault(entry, {}), device, (need + dtype.itemsize - 1) // dtype.itemsize, dtype)
    return ptr(ws), dtype.itemsize * ws.numel()


def _check_info(info, error):
    """Reads an entry's ``info`` word back (synchronises with the stream) and raises ``error(word)`` when it is set"""
    bad = int(info.item())
    if bad:
        raise error(bad)


def _binary_csr_rows(who, csr, rows, n_rows, why):
    """The call shape of the entries that walk a binary resident ``features.DeviceCSR`` and its transpose over ``rows=(r0, r1)`` of
    ``n_rows``: refuses a matrix with values (``why``: the entry's reason) -> the eight leading arguments, ``whole`` of ``_row_range``"""
    if csr.data is not None:
        raise ValueError(f'{who}: {why}; this matrix has values')
    r0, r1, whole = _row_range(rows, n_rows)
    t_indptr, t_indices, _ = csr.transposed()
    return (ptr(csr.indptr), ptr(csr.indices), ptr(t_indptr), ptr(t_indices), *csr.shape, r0, r1), whole


def _f32_rows_view(who, name, t, shape=None, square=False):
    """``(n_rows, n_cols, ld)`` of a float32 matrix view with unit column stride and rows at least a row apart (a dimension of size <= 1
    has no stride to check); ``shape``: the shape it must have; ``square``: any square one, refused in the words of the SPD entries"""
    ok = t.dim() == 2 and (shape is None or tuple(t.shape) == tuple(shape)) and (not square or t.shape[0] == t.shape[1]) \
        and (t.shape[1] <= 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1])
    if square:
        if t.dtype != torch.float32:
            raise ValueError(f'{who}: float32 only, got {t.dtype}')
        if not ok:
            raise ValueError(f'{who}: a square row-major view is needed, got shape {tuple(t.shape)} strides {t.stride()}')
    elif t.dtype != torch.float32 or not ok:
        raise ValueError(f'{who}: {name} must be a float32 {list(shape) if shape else "[n, f]"} view with unit column stride, got {t.dtype} '
                         f'{tuple(t.shape)} strides {t.stride()}')
    n, c = int(t.shape[0]), int(t.shape[1])
    return n, c, (int(t.stride(0)) if n > 1 else max(c, 1))


def _rows_out(who, out, shape, whole, device):
    """``(out, ld)`` of a dense float32 result written by row range: ``out`` checked, or allocated (zeroed unless every row is written)"""
    if out is None:
        out = (torch.empty if whole else torch.zeros)(shape, device=device, dtype=torch.float32)
    return out, _f32_rows_view(who, 'out', out, shape)[2]


def _row_list(rows, n):
    """``(rows as contiguous int64 or None, B)`` of a list of row indices (None: every one of the ``n`` rows)"""
    return (None, n) if rows is None else (rows.long().contiguous(), rows.numel())


# ---- neighbourhood models (csrc/knn.hip) ------------------------------------------------------------------------------------------
KNN_SIM_CODES = {'cosine': 0, 'jaccard': 1, 'asymmetric_cosine': 2, 'sorensen_dice': 3, 'tversky': 4}
KNN_MAX_K = 256


def knn_topk(csr, sim, k: int, shrinkage: float = 0., alpha=None, beta=None, rows=None, tile_cols: int = 0):
    """The ``k`` most similar rows of every row of a binary resident ``features.DeviceCSR`` [n, m] (``compute_similarity_top_k``,
    utilities/similarities.py:18-61, with the similarity of :64-130 named by ``sim``: a key of ``KNN_SIM_CODES`` or its code) ->
    ``(idx int32 [n, k], val float32 [n, k], len int32 [n])``, every list sorted by (value descending, index ascending), (-1, 0) behind
    its length. ``rows=(r0, r1)`` computes that row range only (the other rows come back empty); ``tile_cols`` as in the header."""
    code = KNN_SIM_CODES.get(getattr(sim, 'name', sim), sim)
    if not isinstance(code, int) or code not in KNN_SIM_CODES.values():
        raise ValueError(f'knn_topk: unknown similarity {sim!r} (one of {sorted(KNN_SIM_CODES)})')
    _need_cuda(csr.indptr)
    n, dev = csr.shape[0], csr.indptr.device
    args, whole = _binary_csr_rows('knn_topk', csr, rows, n, 'the similarities are stated for 0/1 data only (utilities/similarities.py:11-15)')
    idx = (torch.empty if whole else partial(torch.full, fill_value=-1))((n, k), device=dev, dtype=torch.int32)
    val = (torch.empty if whole else torch.zeros)((n, k), device=dev, dtype=torch.float32)
    length = (torch.empty if whole else torch.zeros)((n,), device=dev, dtype=torch.int32)
    call('sbr_knn_topk', *args, code, float(0. if alpha is None else alpha), float(0. if beta is None else beta), float(shrinkage), int(k),
         int(tile_cols), ptr(idx), ptr(val), ptr(length), stream())
    return idx, val, length


def dense_knn_topk(F: torch.Tensor, k: int, shrinkage: float = 0., rows=None):
    """The ``k`` most similar rows of every row of a dense float32 matrix ``F`` [n, d] by cosine (``compute_similarity_top_k`` with
    ``dense_compute_cosine_sim_mtx``, utilities/similarities.py:18-61, :86-93; csrc/dense_knn.hip) -> the lists of ``knn_topk``. The
    candidates of a row are the rows with a non-zero dot product, itself included with value +0; values are signed. ``F``: a 2-D CUDA
    view with unit column stride (rows may be further apart than ``d``). ``rows=(r0, r1)`` computes that row range only (the other
    rows come back empty). Refuses a row whose norm is not finite (an inf or NaN entry, or an overflowing sum of squares): reads one
    flag back, which synchronises with the stream."""
    if not (isinstance(k, numbers.Integral) and 1 <= k <= KNN_MAX_K):
        raise ValueError(f'dense_knn_topk: k={k!r} outside [1, {KNN_MAX_K}]')
    if not shrinkage >= 0:
        raise ValueError(f'dense_knn_topk: negative shrinkage {shrinkage}')
    _need_cuda(F)
    n, d, ld = _f32_rows_view('dense_knn_topk', 'F', F)
    r0, r1, whole = _row_range(rows, n, 'dense_knn_topk')
    dev = F.device
    idx = (torch.empty if whole else partial(torch.full, fill_value=-1))((n, k), device=dev, dtype=torch.int32)
    val = (torch.empty if whole else torch.zeros)((n, k), device=dev, dtype=torch.float32)
    length = (torch.empty if whole else torch.zeros)((n,), device=dev, dtype=torch.int32)
    if n == 0:
        return idx, val, length
    norms = torch.empty(n, device=dev, dtype=torch.float32)
    call('sbr_row_norms_f32', ptr(F), n, d, ld, ptr(norms), stream())
    if not bool(torch.isfinite(norms).all()):
        raise ValueError('dense_knn_topk: a row of F has a norm that is not finite (inf / NaN entries, or a sum of squares over the fp32 range)')
    call('sbr_dense_knn_topk', ptr(F), ptr(norms), n, d, ld, r0, r1, float(shrinkage), int(k), ptr(idx), ptr(val), ptr(length), stream())
    return idx, val, length


def _csr_parts(x):
    """(indptr, indices, data or None, shape) of a ``features.DeviceCSR`` or of a plain tuple of that form"""
    if isinstance(x, (tuple, list)):
        return x
    return x.indptr, x.indices, x.data, tuple(x.shape)


def csr_rows_times_csr(x, rows: Optional[torch.Tensor], y, tile_cols: int = 0) -> torch.Tensor:
    """``X[rows] @ Y`` as dense float32 rows [len(rows), Y.shape[1]] with both operands sparse and resident: ``features.DeviceCSR``s or
    ``(indptr int64, indices int32 sorted, data float32 | None = ones, shape)`` tuples — ``matrix @ sim_mtx.T`` and ``sim_mtx @ matrix``
    (algorithms/knn_algs.py:116, :96). ``rows=None``: every row. Fixed summation order (ascending column of X): the same bits on
    every run."""
    xp, xi, xd, xs = _csr_parts(x)
    yp, yi, yd, ys = _csr_parts(y)
    if xs[1] != ys[0]:
        raise ValueError(f'csr_rows_times_csr: shapes {tuple(xs)} and {tuple(ys)} do not chain')
    _need_cuda(xp, yp, rows)
    rows, B = _row_list(rows, xs[0])
    out = torch.empty(B, ys[1], device=xp.device, dtype=torch.float32)
    call('sbr_csr_rows_times_csr', ptr(xp), ptr(xi), ptr(xd), ptr(rows), B, ptr(yp), ptr(yi), ptr(yd), int(ys[1]), int(tile_cols), ptr(out),
         out.stride(0) if B else ys[1], stream())
    return out


# ---- EASE (csrc/ease.hip) ---------------------------------------------------------------------------------------------------------
def gram_dense(csr, diag_add: float = 0., rows=None, tile_cols: int = 0, out=None) -> torch.Tensor:
    """``X^T X + diag_add * I`` of a binary resident ``features.DeviceCSR`` X [n, m] as dense float32 [m, m], counted exactly
    (algorithms/linear_algs.py:150-153). ``rows=(r0, r1)`` computes that row range only (the other rows of a new result are zero, those
    of ``out`` keep what they hold); ``out``: a float32 [m, m] view with unit column stride to write into; ``tile_cols`` as in the header."""
    _need_cuda(csr.indptr, out)
    m = csr.shape[1]
    args, whole = _binary_csr_rows('gram_dense', csr, rows, m, 'the counts are integers for 0/1 data only')
    out, ld = _rows_out('gram_dense', out, (m, m), whole, csr.indptr.device)
    call('sbr_gram_dense', *args, float(diag_add), int(tile_cols), ptr(out), ld, stream())
    return out


def spd_inverse_(A: torch.Tensor) -> torch.Tensor:
    """In-place inverse of a symmetric positive definite float32 matrix (a square row-major view; what lies outside the view is left
    alone) by the blocked symmetric sweep of ``sbr_spd_inverse_f32`` — ``np.linalg.inv(G)``, algorithms/linear_algs.py:155. Fixed
    operation order: the same bits on every run. Raises ``ValueError`` naming the pivot when one is not positive (A then holds no
    inverse). Reads one int32 back: synchronises with the stream."""
    _need_cuda(A)
    n, _, ld = _f32_rows_view('spd_inverse_', 'A', A, square=True)
    if n == 0:
        return A
    info = torch.zeros(1, device=A.device, dtype=torch.int32)
    call('sbr_spd_inverse_f32', ptr(A), n, ld, *_entry_ws(A.device, 'sbr_spd_inverse_f32', n), ptr(info), stream())
    _check_info(info, lambda bad: ValueError(f'spd_inverse_: pivot {bad - 1} is not positive: the matrix is not positive definite in float32'))
    return A


def ease_weights_(P: torch.Tensor) -> torch.Tensor:
    """``B = P / (-diag(P))`` (column j divided by ``-P[j, j]``) with a zero diagonal, in place — algorithms/linear_algs.py:157-158."""
    _need_cuda(P)
    n, _, ld = _f32_rows_view('ease_weights_', 'P', P, square=True)
    if n:
        call('sbr_ease_weights_f32', ptr(P), n, ld, _entry_ws(P.device, 'sbr_spd_inverse_f32', n)[0], stream())
    return P


# ---- SLIM (csrc/slim.hip) ---------------------------------------------------------------------------------------------------------
SLIM_MAX_ITEMS = 40832            # the residual of a column lives in LDS (include/sibrar_hip.h)


def slim_weights(G: torch.Tensor, l1: float, l2: float, max_iter: int, tol: float = 1e-4, cols=None, out=None):
    """The non-negative elastic-net item weights of SLIM (algorithms/linear_algs.py:39-112) from the Gram matrix ``G = X^T X`` (a square
    float32 row view, as ``gram_dense`` counts it) -> ``(W float32 [m, m], n_iter int32 [m])``: column j of ``W`` minimises
    ``1/2 (G_jj - 2 w.q + w.G w) + l1 sum(w) + 1/2 l2 w.w`` over ``w >= 0, w_j = 0`` (``q = G[:, j]``, ``q_j = 0``) by cyclic coordinate
    descent in ascending order, stopped after the sweep with ``max |dw| <= tol * max |w|`` or after ``max_iter`` sweeps (``sbr_slim_cd_f32``;
    the same bits on every run). ``n_iter[j]``: the sweeps of column j, negative when it stopped at ``max_iter`` unconverged.
    ``cols=(c0, c1)`` computes that column range only (the other columns of a new result are zero, those of ``out`` keep what they hold;
    their ``n_iter`` is 0); ``out``: a float32 [m, m] view with unit column stride to write into; it must not overlap ``G``, which the
    kernel reads while it writes ``W`` (refused)."""
    _need_cuda(G, out)
    m, _, ldg = _f32_rows_view('slim_weights', 'G', G, square=True)
    if not (l1 >= 0 and l2 >= 0 and tol >= 0):
        raise ValueError(f'slim_weights: l1={l1!r}, l2={l2!r} and tol={tol!r} must not be negative')
    if not (isinstance(max_iter, numbers.Integral) and max_iter >= 1):
        raise ValueError(f'slim_weights: max_iter={max_iter!r} must be an integer >= 1')
    c0, c1, whole = _row_range(cols, m)
    out, ldw = _rows_out('slim_weights', out, (m, m), whole, G.device)
    if m and ptr(out) < ptr(G) + 4 * ((m - 1) * ldg + m) and ptr(G) < ptr(out) + 4 * ((m - 1) * ldw + m):
        raise ValueError('slim_weights: out overlaps G in memory; the weights cannot be written over the Gram matrix they are solved from')
    n_iter = torch.zeros(m, device=G.device, dtype=torch.int32)
    call('sbr_slim_cd_f32', ptr(G), m, ldg, c0, c1, float(l1), float(l2), int(max_iter), float(tol), ptr(out), ldw, ptr(n_iter), stream())
    return out, n_iter


# ---- P3alpha (csrc/p3alpha.hip) ----------------------------------------------------------------------------------------------------
def p3_walk_dense(csr, rows=None, tile_cols: int = 0, out=None) -> torch.Tensor:
    """The item-item matrix ``W = D_i^-1 X^T D_u^-1 X`` of the three-step random walk on a binary resident ``features.DeviceCSR`` X
    [n, m] as dense float32 [m, m] (algorithms/graph_algs.py:35-59), in the fixed order of ``sbr_p3_walk_dense``: the same bits on every
    run. ``rows``, ``out`` and ``tile_cols`` as in ``gram_dense``."""
    m = csr.shape[1]
    args, whole = _binary_csr_rows('p3_walk_dense', csr, rows, m, 'the walk is stated for 0/1 data only (degrees are entry counts)')
    _need_cuda(csr.indptr, out)
    out, ld = _rows_out('p3_walk_dense', out, (m, m), whole, csr.indptr.device)
    call('sbr_p3_walk_dense', *args, int(tile_cols), ptr(out), ld, stream())
    return out


def p3_score_rows(csr, rows: Optional[torch.Tensor], W: torch.Tensor, alpha: float) -> torch.Tensor:
    """``((D_u^-1 X)[rows] @ W) ** alpha`` as dense float32 rows [len(rows), m] (algorithms/graph_algs.py:59-68) with X a binary resident
    ``features.DeviceCSR`` [n, m] and ``W`` the contiguous float32 [m, m] result of ``p3_walk_dense``. ``rows=None``: every row. Fixed
    summation order (ascending item of the user): the same bits on every run."""
    if csr.data is not None:
        raise ValueError('p3_score_rows: the walk is stated for 0/1 data only (degrees are entry counts); this matrix has values')
    n, m = csr.shape
    if W.dtype != torch.float32 or W.dim() != 2 or tuple(W.shape) != (m, m) or not W.is_contiguous():
        raise ValueError(f'p3_score_rows: W must be a contiguous float32 [{m}, {m}] matrix, got {W.dtype} {tuple(W.shape)} strides {W.stride()}')
    if not float(alpha) > 0:
        raise ValueError(f'p3_score_rows: alpha={alpha!r} must be positive')
    _need_cuda(csr.indptr, rows, W)
    rows, B = _row_list(rows, n)
    out = torch.empty(B, m, device=csr.indptr.device, dtype=torch.float32)
    call('sbr_p3_score_rows', ptr(csr.indptr), ptr(csr.indices), ptr(rows), B, ptr(W), max(m, 1), m, float(alpha), ptr(out), max(m, 1), stream())
    return out


# ---- LightGCN's propagation (csrc/graph_prop.hip) -------------------------------------------------------------------------------------
GRAPH_MAX_D = 512


def _graph_table(who, name, t, shape):
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f'{who}: {name} must be a contiguous float32 {list(shape)} table, got {t.dtype} {tuple(t.shape)} strides {t.stride()}')


def _graph_propagate(who, csr, x, out, sum, sum_scale, rows, noise=None):
    """the launch behind ``graph_propagate`` and ``graph_propagate_noise`` (``noise``: (eps, seed, stream_id))"""
    if csr.data is not None:
        raise ValueError(f'{who}: the normalised adjacency is stated for 0/1 data only (degrees are entry counts); this matrix has values')
    _need_cuda(csr.indptr, x, out, sum)
    n_users, n_items = csr.shape
    n = n_users + n_items
    if x.dim() != 2:
        raise ValueError(f'{who}: x must be a table [{n}, D], got shape {tuple(x.shape)}')
    shape = (n, int(x.shape[1]))
    _graph_table(who, 'x', x, shape)
    r0, r1, whole = _row_range(rows, n)
    if out is None:
        out = (torch.empty if whole else torch.zeros)(shape, device=x.device, dtype=torch.float32)
    _graph_table(who, 'out', out, shape)
    if sum is not None:
        _graph_table(who, 'sum', sum, shape)
    t_indptr, t_indices, _ = csr.transposed()
    args = (ptr(csr.indptr), ptr(csr.indices), ptr(t_indptr), ptr(t_indices), n_users, n_items, r0, r1, ptr(x), ptr(out), ptr(sum),
            float(sum_scale), shape[1])
    if noise is None:
        call('sbr_graph_propagate_f32', *args, stream())
    else:
        call('sbr_graph_propagate_noise_f32', *args, *noise, stream())
    return out


def graph_propagate(csr, x: torch.Tensor, out=None, sum=None, sum_scale: float = 1.0, rows=None) -> torch.Tensor:
    """``y = A^ x`` with ``A^ = D^-1/2 A D^-1/2`` the normalised adjacency of the bipartite graph of a binary resident
    ``features.DeviceCSR`` [n_users, n_items], over the joint row space (users first, then items): ``x`` and the result are contiguous
    float32 [n_users + n_items, D], D <= 512 — ``sbr_graph_propagate_f32``: one fmaf chain per element in ascending CSR order, the same
    bits on every run and for every split of the rows. ``sum``: a table of the same shape that becomes ``(sum + y) * sum_scale`` in the
    same launch (LightGCN's running layer sum). ``rows=(r0, r1)`` computes that range of joint rows only; ``out``: a table to write into
    (the rows outside the range keep what they hold; those of a new result are zero). ``x`` may not be ``out`` or ``sum``."""
    return _graph_propagate('graph_propagate', csr, x, out, sum, sum_scale, rows)


def graph_propagate_noise(csr, x: torch.Tensor, eps: float, seed: int, stream_id: int, out=None, sum=None, sum_scale: float = 1.0,
                          rows=None) -> torch.Tensor:
    """``graph_propagate`` with the perturbation of SimGCL / XSimGCL applied in the same launch (``sbr_graph_propagate_noise_f32``):
    ``y = p + sign(p) * eps * u / |u_row|`` with ``p = A^ x`` and ``u = U(seed, stream_id, row, column)`` in [0, 1) from Philox4x32-10,
    generated in registers — a pure function of its four arguments, so the same bits on every run and for every split of the rows.
    ``sum`` takes the perturbed ``y``. ``eps = 0`` is ``graph_propagate`` bit for bit. ``seed`` and ``stream_id`` are integers in
    [0, 2^64); the other arguments are ``graph_propagate``'s."""
    who = 'graph_propagate_noise'
    for name, v in (('seed', seed), ('stream_id', stream_id)):
        if int(v) != v or not 0 <= v < 1 << 64:
            raise ValueError(f'{who}: {name}={v!r} must be an integer in [0, 2^64)')
    return _graph_propagate(who, csr, x, out, sum, sum_scale, rows, noise=(float(eps), int(seed), int(stream_id)))


_GRAPH_WS = ({}, {})              # slot -> device -> the ping-pong tables of LightGCNPropagateFn


def _lightgcn_mean(csr, e0: torch.Tensor, n_layers: int) -> torch.Tensor:
    """``(1 / (L + 1)) sum_{k=0..L} A^^k e0`` for L >= 1: the sum is seeded with ``e0``, layer k reads one scratch table and writes the
    other, and every launch adds its layer to the sum (the last one also scales it)"""
    acc = e0.clone()
    x = e0
    for k in range(1, n_layers + 1):
        y = _device_ws(_GRAPH_WS[k & 1], e0.device, e0.numel(), torch.float32)[:e0.numel()].view(e0.shape)
        graph_propagate(csr, x, out=y, sum=acc, sum_scale=1.0 if k < n_layers else 1.0 / (n_layers + 1))
        x = y
    return acc


class LightGCNPropagateFn(Function):
    """LightGCN's layer combination (He et al., SIGIR 2020, equations 8 and 10 with alpha_k = 1 / (L + 1)):
    ``E = (1 / (L + 1)) sum_{k=0..L} A^^k E0`` for the joint table ``E0`` [n_users + n_items, D] — L launches of
    ``sbr_graph_propagate_f32``. ``A^`` is symmetric, so the backward pass is the same computation on the incoming gradient. ``L = 0``
    returns ``E0`` and launches nothing. Fixed order, no atomics: valid in deterministic mode."""

    @staticmethod
    def forward(ctx, csr, e0, n_layers: int):
        n_layers = int(n_layers)
        if n_layers < 0:
            raise ValueError(f'LightGCNPropagateFn: n_layers={n_layers} is negative')
        ctx.csr, ctx.n_layers = csr, n_layers
        if n_layers == 0:
            return e0.view_as(e0)
        _need_cuda(e0)
        return _lightgcn_mean(csr, _f32c(e0), n_layers)

    @staticmethod
    def backward(ctx, g):
        if ctx.n_layers == 0:
            return None, g, None
        return None, _lightgcn_mean(ctx.csr, _f32c(g), ctx.n_layers), None


GRAPH_NOISE_MAX_LAYERS, GRAPH_NOISE_MAX_VIEWS = 64, 4             # stream_id = step * 256 + view * 64 + layer


def noise_stream_id(step: int, view: int, layer: int) -> int:
    """the ``stream_id`` from which layer ``layer`` of view ``view`` of training step ``step`` draws its noise"""
    if not 0 <= layer < GRAPH_NOISE_MAX_LAYERS or not 0 <= view < GRAPH_NOISE_MAX_VIEWS or not 0 <= step < 1 << 56:
        raise ValueError(f'noise_stream_id: layer={layer} outside [0, {GRAPH_NOISE_MAX_LAYERS}), view={view} outside '
                         f'[0, {GRAPH_NOISE_MAX_VIEWS}) or step={step} outside [0, 2^56)')
    return step * 256 + view * 64 + layer


def _graph_scratch(slot, like):
    return _device_ws(_GRAPH_WS[slot], like.device, like.numel(), torch.float32)[:like.numel()].view(like.shape)


class NoisyPropagateFn(Function):
    """The layer stack of SimGCL / XSimGCL: ``E_k = perturb_k(A^ E_(k-1))`` with ``E_0 = e0`` [n_users + n_items, D] and ``perturb_k`` the
    noise of ``graph_propagate_noise`` drawn from ``stream_id = step * 256 + view * 64 + k`` -> ``(mean, kept)`` with
    ``mean = (1 / L) sum_{k=1..L} E_k`` (layer 0 is left out, as in the authors' code) and ``kept = E_keep_layer`` (``keep_layer=None``:
    None). L launches: the running sum starts at zero and every launch adds its perturbed layer (the last one also scales by 1 / L).
    ``eps = 0`` runs ``sbr_graph_propagate_f32``, which gives the same bits as the noisy entry at eps = 0.

    Backward: the noise is a constant and the sign has derivative zero, so the derivative is the linear operator alone. With
    ``c_k = g_mean * (1 / L) + [k == keep_layer] g_kept``, ``dE0 = A^(c_1 + A^(c_2 + ... A^ c_L))``, by Horner: ``t = c_L``; for
    k = L .. 2, ``t = (c_(k-1) + A^ t) * 1`` through the ``sum`` epilogue of ``sbr_graph_propagate_f32``; ``dE0 = A^ t`` — L launches of
    the existing entry, no kernel of its own. Fixed order, no atomics: valid in deterministic mode."""

    @staticmethod
    def forward(ctx, csr, e0, n_layers: int, eps: float, seed: int, step: int, view: int, keep_layer=None):
        n_layers = int(n_layers)
        if n_layers < 1:
            raise ValueError(f'NoisyPropagateFn: n_layers={n_layers}: with no layer there is nothing to perturb')
        if keep_layer is not None and not 1 <= keep_layer <= n_layers:
            raise ValueError(f'NoisyPropagateFn: keep_layer={keep_layer} outside [1, {n_layers}]')
        if not float(eps) >= 0:
            raise ValueError(f'NoisyPropagateFn: eps={eps} is negative')
        ids = [noise_stream_id(int(step), int(view), k) for k in range(1, n_layers + 1)]
        _need_cuda(e0)
        x = _f32c(e0)
        ctx.csr, ctx.n_layers, ctx.keep_layer = csr, n_layers, keep_layer
        ctx.set_materialize_grads(False)
        acc, kept = torch.zeros_like(x), None
        for k in range(1, n_layers + 1):
            y = torch.empty_like(x) if k == keep_layer else _graph_scratch(k & 1, x)
            scale = 1.0 if k < n_layers else 1.0 / n_layers
            if eps == 0:
                graph_propagate(csr, x, out=y, sum=acc, sum_scale=scale)
            else:
                graph_propagate_noise(csr, x, eps, seed, ids[k - 1], out=y, sum=acc, sum_scale=scale)
            x = y
            if k == keep_layer:
                kept = y
        return acc, kept

    @staticmethod
    def backward(ctx, g_mean, g_kept=None):
        if g_mean is None and g_kept is None:
            return (None,) * 8
        L, keep = ctx.n_layers, ctx.keep_layer
        gm = None if g_mean is None else _f32c(g_mean) * (1.0 / L)
        gk = None if g_kept is None else _f32c(g_kept)

        def c(k):                                                    # a table of its own: it becomes the launch's running sum
            if gk is not None and k == keep:
                return gk.clone() if gm is None else gm + gk
            return torch.zeros_like(gk) if gm is None else gm.clone()

        t = c(L)
        for k in range(L, 1, -1):
            s = c(k - 1)
            graph_propagate(ctx.csr, t, out=_graph_scratch(k & 1, t), sum=s, sum_scale=1.0)
            t = s
        return (None, graph_propagate(ctx.csr, t)) + (None,) * 6


# ---- NGCF's layer (csrc/ngcf.hip) -------------------------------------------------------------------------------------------------------
NGCF_MAX_WIDTH = 128


def _ngcf_slice(who, name, t, n, d):
    """a float32 [n, d] column slice of a wider row-major table (or a contiguous table) -> its leading dimension"""
    if t.dtype != torch.float32 or tuple(t.shape) != (n, d) or (d > 1 and t.stride(1) != 1) or (n > 1 and t.stride(0) < d):
        raise ValueError(f'{who}: {name} must be float32 {[n, d]} with unit column stride (a column slice of a row-major table), got '
                         f'{t.dtype} {tuple(t.shape)} strides {t.stride()}')
    return max(int(t.stride(0)), d) if n > 1 else d


def _ngcf_operands(who, csr, x, W1, W2, slope, p, seed, stream_id):
    if csr.data is not None:
        raise ValueError(f'{who}: the normalised adjacency is stated for 0/1 data only (degrees are entry counts); this matrix has values')
    n_users, n_items = csr.shape
    n = n_users + n_items
    if x.dim() != 2 or W1.dim() != 2:
        raise ValueError(f'{who}: x must be a table [{n}, Din] and W1 a matrix [Din, Dout], got shapes {tuple(x.shape)} and {tuple(W1.shape)}')
    din, dout = int(W1.shape[0]), int(W1.shape[1])
    if not (1 <= din <= NGCF_MAX_WIDTH and 1 <= dout <= NGCF_MAX_WIDTH):
        raise ValueError(f'{who}: widths Din={din}, Dout={dout} outside [1, {NGCF_MAX_WIDTH}]')
    _graph_table(who, 'x', x, (n, din))
    _graph_table(who, 'W1', W1, (din, dout))
    _graph_table(who, 'W2', W2, (din, dout))
    for name, v in (('seed', seed), ('stream_id', stream_id)):
        if int(v) != v or not 0 <= v < 1 << 64:
            raise ValueError(f'{who}: {name}={v!r} must be an integer in [0, 2^64)')
    t_indptr, t_indices, _ = csr.transposed()
    graph = (ptr(csr.indptr), ptr(csr.indices), ptr(t_indptr), ptr(t_indices), n_users, n_items)
    return graph, n, din, dout, (float(slope), float(p), int(seed), int(stream_id))


def ngcf_layer(csr, x: torch.Tensor, W1: torch.Tensor, W2: torch.Tensor, bias: torch.Tensor, slope: float = 0.2, p: float = 0.0,
               seed: int = 0, stream_id: int = 0, h=None, out=None, rows=None):
    """One NGCF layer over the joint row space of a binary resident ``features.DeviceCSR`` in one launch (``sbr_ngcf_layer_fwd``):
    ``s = A^ x``, ``z = (s + x) W1 + (s * x) W2 + bias``, ``h = dropout_p(LeakyReLU_slope(z))``, ``out = h / max(|h|, 1e-12)`` row-wise
    -> ``(h, out)``. ``x`` [n, Din], ``W1`` / ``W2`` [Din, Dout] and ``bias`` [Dout] are contiguous float32, widths up to 128; ``h`` is a
    contiguous [n, Dout] table to write into, ``out`` may be a column slice of a wider row-major table (the concatenated representation:
    nothing outside the slice is written). The dropout mask is Philox4x32-10 of ``(seed, stream_id, row, column)``; ``p = 0`` draws
    nothing. Fixed order, no atomics: the same bits on every run and for every split of the rows (``rows=(r0, r1)``; rows outside
    keep what they hold, those of a new result are zero). No CPU fallback."""
    who = 'ngcf_layer'
    _need_cuda(csr.indptr, x, W1, W2, bias, h, out)
    graph, n, din, dout, tail = _ngcf_operands(who, csr, x, W1, W2, slope, p, seed, stream_id)
    _graph_table(who, 'bias', bias, (dout,))
    r0, r1, whole = _row_range(rows, n)
    make = torch.empty if whole else torch.zeros
    if h is None:
        h = make((n, dout), device=x.device, dtype=torch.float32)
    if out is None:
        out = make((n, dout), device=x.device, dtype=torch.float32)
    _graph_table(who, 'h', h, (n, dout))
    ld = _ngcf_slice(who, 'out', out, n, dout)
    call('sbr_ngcf_layer_fwd', *graph, r0, r1, ptr(x), din, ptr(W1), ptr(W2), ptr(bias), dout, *tail, ptr(h), ptr(out), ld, stream())
    return h, out


def ngcf_layer_bwd(csr, x: torch.Tensor, W1: torch.Tensor, W2: torch.Tensor, h: torch.Tensor, g_out: torch.Tensor, g_h=None,
                   slope: float = 0.2, p: float = 0.0, seed: int = 0, stream_id: int = 0, rows=None):
    """The backward pass of ``ngcf_layer`` (``sbr_ngcf_layer_bwd``) from the layer's input ``x``, its output ``h`` and the gradients
    ``g_out`` (of ``out``; may be a column slice) and ``g_h`` (of ``h``, from the next layer; None for the last)
    -> ``(ds, dx_direct, dW1, dW2, dbias)``: the gradient of ``x`` is ``dx_direct + A^ ds`` (``graph_propagate(csr, ds, sum=dx_direct)``).
    The gather, the mask and the norm are recomputed. The weight gradients are per-workgroup partials folded in workgroup order: no
    atomics, the same bits on every run."""
    who = 'ngcf_layer_bwd'
    _need_cuda(csr.indptr, x, W1, W2, h, g_out, g_h)
    graph, n, din, dout, tail = _ngcf_operands(who, csr, x, W1, W2, slope, p, seed, stream_id)
    _graph_table(who, 'h', h, (n, dout))
    if g_h is not None:
        _graph_table(who, 'g_h', g_h, (n, dout))
    ld = _ngcf_slice(who, 'g_out', g_out, n, dout)
    r0, r1, whole = _row_range(rows, n)
    make = torch.empty if whole else torch.zeros
    ds, dxd = (make((n, din), device=x.device, dtype=torch.float32) for _ in range(2))
    dW1, dW2 = (torch.zeros((din, dout), device=x.device, dtype=torch.float32) for _ in range(2))
    dbias = torch.zeros(dout, device=x.device, dtype=torch.float32)
    ws, ws_bytes = _entry_ws(x.device, 'sbr_ngcf_layer_bwd', r1 - r0, din, dout)
    call('sbr_ngcf_layer_bwd', *graph, r0, r1, ptr(x), din, ptr(W1), ptr(W2), dout, *tail, ptr(h), ptr(g_out), ld, ptr(g_h), ptr(ds), ptr(dxd),
         ptr(dW1), ptr(dW2), ptr(dbias), ws, ws_bytes, stream())
    return ds, dxd, dW1, dW2, dbias


def _ngcf_input_grad(csr, x, W1, W2, h, g_out, g_h, tail):
    """-> (dx, dW1, dW2, dbias) of one layer: the fused backward launch, then the graph part of dx through the propagation's ``sum``"""
    ds, dxd, dW1, dW2, dbias = ngcf_layer_bwd(csr, x, W1, W2, h, g_out, g_h, *tail)
    graph_propagate(csr, ds, out=_graph_scratch(0, ds), sum=dxd, sum_scale=1.0)
    return dxd, dW1, dW2, dbias


class NGCFLayerFn(Function):
    """One NGCF layer on the autograd tape: ``(h, out) = NGCFLayerFn.apply(csr, x, W1, W2, bias, slope, p, seed, stream_id)`` as
    ``ngcf_layer`` computes them. Backward: one ``sbr_ngcf_layer_bwd`` launch and one ``sbr_graph_propagate_f32`` (A^ is symmetric).
    Fixed order, no atomics: valid in deterministic mode."""

    @staticmethod
    def forward(ctx, csr, x, W1, W2, bias, slope: float = 0.2, p: float = 0.0, seed: int = 0, stream_id: int = 0):
        x, W1, W2, bias = _f32c(x), _f32c(W1), _f32c(W2), _f32c(bias)
        h, out = ngcf_layer(csr, x, W1, W2, bias, slope, p, seed, stream_id)
        ctx.csr, ctx.tail = csr, (float(slope), float(p), int(seed), int(stream_id))
        ctx.save_for_backward(x, W1, W2, h)
        return h, out

    @staticmethod
    def backward(ctx, g_h, g_out):
        x, W1, W2, h = ctx.saved_tensors
        dx, dW1, dW2, dbias = _ngcf_input_grad(ctx.csr, x, W1, W2, h, _f32c(g_out), _f32c(g_h), ctx.tail)
        return (None, dx, dW1, dW2, dbias) + (None,) * 4


class NGCFPropagateFn(Function):
    """NGCF's layer stack: ``table = NGCFPropagateFn.apply(csr, e0, slope, p, seed, W1_1, W2_1, bias_1, ..., W1_L, W2_L, bias_L)`` is
    ``[e0 | normalize(E_1) | ... | normalize(E_L)]`` [n, D0 + sum of the layer widths] with ``E_l`` the ``h`` of ``ngcf_layer`` on
    ``E_(l-1)``: L launches, every layer writes its normalised rows straight into its column slice. Layer l (1-based) draws its
    dropout from ``stream_id = l``. Backward: per layer, from the last, one ``sbr_ngcf_layer_bwd`` on the slice of the incoming
    gradient and the gradient the next layer sent back, and one ``sbr_graph_propagate_f32``. No layer returns ``e0`` and launches
    nothing."""

    @staticmethod
    def forward(ctx, csr, e0, slope, p, seed, *params):
        if len(params) % 3:
            raise ValueError('NGCFPropagateFn: the parameters come as (W1, W2, bias) per layer')
        n_layers = len(params) // 3
        ctx.csr, ctx.n_layers = csr, n_layers
        if n_layers == 0:
            return e0.view_as(e0)
        _need_cuda(e0)
        x = _f32c(e0)
        params = [_f32c(t) for t in params]
        widths = [int(x.shape[1])] + [int(params[3 * k].shape[1]) for k in range(n_layers)]
        table = torch.empty((x.shape[0], sum(widths)), device=x.device, dtype=torch.float32)
        table[:, :widths[0]] = x
        saved, off = [x], widths[0]
        for k in range(n_layers):
            W1, W2, bias = params[3 * k:3 * k + 3]
            x, _ = ngcf_layer(csr, x, W1, W2, bias, slope, p, seed, k + 1, out=table[:, off:off + widths[k + 1]])
            saved.append(x)
            off += widths[k + 1]
        ctx.tail, ctx.widths = (float(slope), float(p), int(seed)), widths
        ctx.save_for_backward(*saved, *params)
        return table

    @staticmethod
    def backward(ctx, g):
        if ctx.n_layers == 0:
            return (None, g) + (None,) * 3
        L, widths = ctx.n_layers, ctx.widths
        xs, params = ctx.saved_tensors[:L + 1], ctx.saved_tensors[L + 1:]
        g = _f32c(g)
        grads, dx, off = [None] * (3 * L), None, sum(widths)
        for k in range(L - 1, -1, -1):
            off -= widths[k + 1]
            W1, W2 = params[3 * k], params[3 * k + 1]
            dx, dW1, dW2, dbias = _ngcf_input_grad(ctx.csr, xs[k], W1, W2, xs[k + 1], g[:, off:off + widths[k + 1]], dx, ctx.tail + (k + 1,))
            grads[3 * k:3 * k + 3] = dW1, dW2, dbias
        return (None, g[:, :widths[0]] + dx, None, None, None, *grads)


# ---- the multinomial log-likelihood of Mult-VAE / Mult-DAE (csrc/multinomial.hip) ------------------------------------------------------
def _multinomial_nll(who, csr, rows, logits, grad_scale, inplace):
    """the launch behind ``multinomial_nll`` and ``MultinomialNLLFn``; nothing here synchronises"""
    if csr.data is not None:
        raise ValueError(f'{who}: the multinomial likelihood is stated for 0/1 data only (the targets are the rows\' entries); this matrix has values')
    _need_cuda(csr.indptr, rows, logits)
    n_users, n_items = csr.shape
    if rows.dtype != torch.int64 or rows.dim() != 1 or not rows.is_contiguous():
        raise ValueError(f'{who}: rows must be a contiguous int64 vector, got {rows.dtype} {tuple(rows.shape)}')
    B = rows.numel()
    if logits.dtype != torch.float32 or tuple(logits.shape) != (B, n_items) or not logits.is_contiguous():
        raise ValueError(f'{who}: logits must be a contiguous float32 [{B}, {n_items}] matrix, got {logits.dtype} {tuple(logits.shape)} '
                         f'strides {logits.stride()}')
    if inplace and grad_scale is None:
        raise ValueError(f'{who}: inplace=True writes the gradient over the logits and needs a grad_scale')
    row_loss = torch.empty(B, device=logits.device, dtype=torch.float32)
    row_lse = torch.empty(B, device=logits.device, dtype=torch.float32)
    dlogits = None if grad_scale is None else (logits if inplace else torch.empty_like(logits))
    call('sbr_multinomial_nll_f32', ptr(csr.indptr), ptr(csr.indices), ptr(rows), B, n_items, ptr(logits), ptr(dlogits),
         0.0 if grad_scale is None else float(grad_scale), ptr(row_loss), ptr(row_lse), stream())
    return row_loss, row_lse, dlogits


def multinomial_nll(csr, rows: torch.Tensor, logits: torch.Tensor, grad_scale: Optional[float] = None, inplace: bool = False):
    """The multinomial log-likelihood of Mult-VAE / Mult-DAE (Liang et al., WWW 2018) of the logit rows ``logits`` [B, n_items] against
    the rows ``rows`` (int64 [B]) of a binary resident ``features.DeviceCSR`` [n_users, n_items] — ``sbr_multinomial_nll_f32``, one
    launch: ``row_loss[b] = n_b * logsumexp(logits[b]) - sum of logits[b] at the user's items`` and ``row_lse[b]`` the logsumexp. With a
    ``grad_scale`` the gradient ``grad_scale * (n_b * softmax(logits[b]) - the user's 0/1 row)`` comes back as a third result: a new
    matrix, or ``logits`` itself, overwritten, with ``inplace=True``. A user without items gives a zero loss and a zero gradient row.
    Fixed order (it depends on n_items alone), no atomics: valid in deterministic mode. The row ids are checked here (one
    synchronisation); ``MultinomialNLLFn`` does not check them."""
    if rows.numel() and not (0 <= int(rows.min()) and int(rows.max()) < csr.shape[0]):
        raise ValueError(f'multinomial_nll: row ids outside [0, {csr.shape[0]})')
    row_loss, row_lse, dlogits = _multinomial_nll('multinomial_nll', csr, rows, logits, grad_scale, inplace)
    return (row_loss, row_lse) if grad_scale is None else (row_loss, row_lse, dlogits)


class MultinomialNLLFn(Function):
    """``mean_b row_loss[b]`` of ``multinomial_nll`` as a scalar on the autograd tape. One launch of ``sbr_multinomial_nll_f32`` in the
    forward pass computes the loss and, when the logits need a gradient, the gradient ``(1 / B) (n_b softmax - targets)`` with it; the
    backward pass launches nothing. ``inplace=True`` is the caller's promise that nothing reads the logits after this call, the backward
    pass of their producer included (``LinearActFn`` without an activation does not): the gradient is then written over them
    (``dlogits == logits``). Otherwise, and whenever the logits need no gradient, the logits are left as they are and the gradient, if
    any, is a new matrix. ``unit_upstream=True`` is the promise that the result enters the objective with weight 1: the backward pass
    then hands the stored gradient on as it is; otherwise it is multiplied by the upstream gradient (no synchronisation either way).
    The row ids must lie inside the matrix; they are not checked here (that would synchronise)."""

    @staticmethod
    def forward(ctx, csr, rows, logits, inplace: bool = False, unit_upstream: bool = False):
        need = ctx.needs_input_grad[2]
        B = rows.numel()
        if B == 0:
            raise ValueError('MultinomialNLLFn: an empty batch has no mean')
        row_loss, _, dlogits = _multinomial_nll('MultinomialNLLFn', csr, rows, logits.detach() if logits.is_contiguous() else _f32c(logits.detach()),
                                                1.0 / B if need else None, bool(inplace) and need and logits.is_contiguous())
        ctx.dlogits, ctx.unit_upstream = dlogits, bool(unit_upstream)
        return row_loss.sum() / B

    @staticmethod
    def backward(ctx, g):
        dl, ctx.dlogits = ctx.dlogits, None
        if dl is not None and not ctx.unit_upstream:
            dl = dl.mul_(g)
        return None, None, dl, None, None


# ---- RecVAE's row-wise tails (csrc/recvae.hip) -------------------------------------------------------------------------------------------
ROW_TAIL_MAX_W = 1024             # the widest row of the swish-LayerNorm and prior-KL kernels (a wave keeps the row in registers)


def _row_tail_matrix(who, name, t, shape=None):
    """``t`` as the kernels take it: a contiguous float32 [B, W] matrix on the device (the width's range is the library's refusal)"""
    _need_cuda(t)
    if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        want = 'matrix' if shape is None else f'{list(shape)} matrix'
        raise ValueError(f'{who}: {name} must be a contiguous float32 {want}, got {t.dtype} {tuple(t.shape)} strides {t.stride()}')
    return t


def _row_tail_vector(who, name, t, n):
    _need_cuda(t)
    if t.dtype != torch.float32 or tuple(t.shape) != (n,) or not t.is_contiguous():
        raise ValueError(f'{who}: {name} must be a contiguous float32 [{n}] vector, got {t.dtype} {tuple(t.shape)}')
    return t


def swish_ln_slabs(B: int) -> int:
    """how many slabs of column partials ``sbr_swish_ln_bwd`` writes for ``B`` rows (``sbr_swish_ln_slabs``)"""
    return int(lib().sbr_swish_ln_slabs(int(B)))


class SwishLayerNormFn(Function):
    """One layer tail of RecVAE's encoder, ``sbr_swish_ln_fwd`` / ``sbr_swish_ln_bwd``: with ``s = a + r_in`` (``r_in`` None: ``s = a``),
    ``h = LayerNorm(s * sigmoid(s))`` over the row (biased variance, ``gamma``, ``beta``, ``eps``) and ``r_out = r_in + h``, the running
    sum of the layers' outputs -> ``(h, r_out)``; ``want_sum=False``: ``r_out`` is None and is not computed. One launch forward; two
    backward (the rows, then the slabs of ``d gamma`` / ``d beta`` in slab order). Fixed order, no atomics: valid in deterministic mode.
    ``a`` and ``r_in`` are contiguous float32 [B, H] with 1 <= H <= 1024 (the library refuses other widths)."""

    @staticmethod
    def forward(ctx, a, r_in, gamma, beta, eps: float = 0.1, want_sum: bool = True):
        who = 'SwishLayerNormFn'
        a = _row_tail_matrix(who, 'a', _f32c(a.detach()))
        B, H = a.shape
        if r_in is not None:
            r_in = _row_tail_matrix(who, 'r_in', _f32c(r_in.detach()), (B, H))
        gamma, beta = _row_tail_vector(who, 'gamma', gamma.detach(), H), _row_tail_vector(who, 'beta', beta.detach(), H)
        s, h = torch.empty_like(a), torch.empty_like(a)
        r_out = torch.empty_like(a) if want_sum else None
        mean, rstd = (torch.empty(B, device=a.device, dtype=torch.float32) for _ in range(2))
        call('sbr_swish_ln_fwd', ptr(a), ptr(r_in), ptr(gamma), ptr(beta), float(eps), B, H, ptr(s), ptr(h), ptr(r_out), ptr(mean), ptr(rstd),
             stream())
        ctx.save_for_backward(s, mean, rstd, gamma)
        ctx.has_sum_in = r_in is not None
        ctx.set_materialize_grads(False)
        return h, r_out

    @staticmethod
    def backward(ctx, dh, dr_out):
        s, mean, rstd, gamma = ctx.saved_tensors
        if dh is None and dr_out is None:
            return (None,) * 6
        B, H = s.shape
        dh, dr_out = (None if t is None else _f32c(t) for t in (dh, dr_out))
        da = torch.empty_like(s)
        dr_in = torch.empty_like(s) if (ctx.has_sum_in and ctx.needs_input_grad[1] and dr_out is not None) else None
        dgamma = dbeta = part = None
        if B and (ctx.needs_input_grad[2] or ctx.needs_input_grad[3]):
            dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
            part = torch.empty(swish_ln_slabs(B) * 2 * H, device=s.device, dtype=torch.float32)
        call('sbr_swish_ln_bwd', ptr(s), ptr(mean), ptr(rstd), ptr(gamma), ptr(dh), ptr(dr_out), B, H, ptr(da), ptr(dr_in), ptr(dgamma),
             ptr(dbeta), ptr(part), stream())
        if ctx.has_sum_in and dr_in is None:
            dr_in = da                                                     # no dr_out: dr_in is ds itself
        return da, dr_in if ctx.has_sum_in else None, dgamma, dbeta, None, None


class CompositePriorKLFn(Function):
    """RecVAE's reparameterisation and KL term against its composite prior, ``sbr_prior_kl_fwd`` / ``sbr_prior_kl_bwd`` (one launch each):
    ``z = mu + eps * exp(logvar / 2)`` and ``kl = mean_b weight_b * sum_j (log N(z; mu, logvar) - log p(z))`` with ``p`` the mixture
    3/20 N(0, 1) + 3/4 N(mu_old, exp(logvar_old)) + 1/10 N(0, exp(10)) -> ``(z, kl)``. Gradients go to ``mu`` and ``logvar`` only, from
    the ``z`` that the decoder used and from ``kl``; the upstream gradient of ``kl`` is read on the device (no synchronisation). All
    operands are contiguous float32 [B, L] (``weight``: [B]) with 1 <= L <= 1024. Fixed order, no atomics: valid in deterministic mode."""

    @staticmethod
    def forward(ctx, mu, logvar, eps, mu_old, logvar_old, weight):
        who = 'CompositePriorKLFn'
        mu = _row_tail_matrix(who, 'mu', _f32c(mu.detach()))
        B, L = mu.shape
        if B == 0:
            raise ValueError('CompositePriorKLFn: an empty batch has no mean')
        logvar, eps, mu_old, logvar_old = (_row_tail_matrix(who, n, _f32c(t.detach()), (B, L)) for n, t in (
            ('logvar', logvar), ('eps', eps), ('mu_old', mu_old), ('logvar_old', logvar_old)))
        weight = _row_tail_vector(who, 'weight', weight.detach(), B)
        z = torch.empty_like(mu)
        row_kl = torch.empty(B, device=mu.device, dtype=torch.float32)
        call('sbr_prior_kl_fwd', ptr(mu), ptr(logvar), ptr(eps), ptr(mu_old), ptr(logvar_old), ptr(weight), B, L, ptr(z), ptr(row_kl), stream())
        ctx.save_for_backward(logvar, eps, mu_old, logvar_old, weight, z)
        ctx.set_materialize_grads(False)
        return z, row_kl.sum() / B

    @staticmethod
    def backward(ctx, dz, dkl):
        logvar, eps, mu_old, logvar_old, weight, z = ctx.saved_tensors
        if dz is None and dkl is None:
            return (None,) * 6
        B, L = z.shape
        dz = None if dz is None else _f32c(dz)
        dkl = None if dkl is None else dkl.to(torch.float32).reshape(1)
        dmu, dlogvar = torch.empty_like(z), torch.empty_like(z)
        call('sbr_prior_kl_bwd', ptr(logvar), ptr(eps), ptr(mu_old), ptr(logvar_old), ptr(weight), ptr(z), ptr(dz), ptr(dkl),
             1.0 / B if dkl is not None else 0.0, B, L, ptr(dmu), ptr(dlogvar), stream())
        return dmu, dlogvar, None, None, None, None


# ---- DirectAU's loss terms (csrc/directau.hip) -----------------------------------------------------------------------------------------
UNIFORMITY_MAX_D = 256            # the backward pass keeps a row tile's [64, D] accumulator in registers


def _uniformity_x(who, x, t):
    """-> (x as contiguous float32, n, D, t) of the operand of the uniformity entries; the shape and range refusals are the library's"""
    _need_cuda(x)
    if x.dim() != 2:
        raise ValueError(f'{who}: x must be a matrix [n, D], got shape {tuple(x.shape)}')
    return _f32c(x), int(x.shape[0]), int(x.shape[1]), float(t)


def _uniformity_fwd(who, x, t, max_wg):
    x, n, D, t = _uniformity_x(who, x, t)
    out = torch.empty(2, device=x.device, dtype=torch.float32)                # (S, loss)
    ws, ws_bytes = _entry_ws(x.device, 'sbr_uniformity', n, D, dtype=torch.float64)
    call('sbr_uniformity_fwd', ptr(x), n, D, t, ptr(out), ptr(out) + 4, ws, ws_bytes, int(max_wg), stream())
    return x, out[1], out[0]


def _uniformity_bwd(x, t, S, g, max_wg):
    dx = torch.empty_like(x)
    g = g.reshape(()).to(torch.float32).contiguous()
    call('sbr_uniformity_bwd', ptr(x), x.shape[0], x.shape[1], float(t), ptr(S), ptr(g), ptr(dx), int(max_wg), stream())
    return dx


def uniformity(x: torch.Tensor, t: float = 2.0, max_wg: int = 0):
    """``(loss, S)`` of the uniformity term of DirectAU (Wang et al., KDD 2022) over the rows of ``x`` [n, D], n >= 2, D <= 256, t > 0:
    ``S = sum_{i<j} exp(-t |x_i - x_j|^2)`` and ``loss = log(S * 2 / (n (n - 1)))``, two float32 scalars on the device —
    ``sbr_uniformity_fwd``: the pair weights are formed on chip from 64 x 64 Gram tiles and nothing of size n x n is written. torch's
    ``pdist(x).pow(2).mul(-t).exp().mean().log()``. Equal rows are ordinary pairs; the rows need not be normalised, but ``t * max d^2``
    must stay below 80. ``max_wg``: the most workgroups (0: the default); the bits do not depend on it, on the run or on the mode."""
    _, loss, S = _uniformity_fwd('uniformity', x, t, max_wg)
    return loss, S


class UniformityFn(Function):
    """``ops.uniformity``'s loss on the autograd tape. The forward pass saves ``x`` and ``S``; the backward pass recomputes the pair
    weights (``sbr_uniformity_bwd``) and reads the upstream gradient from device memory: no synchronisation. Fixed order, no atomics:
    valid in deterministic mode."""

    @staticmethod
    def forward(ctx, x, t: float = 2.0, max_wg: int = 0):
        xc, loss, S = _uniformity_fwd('UniformityFn', x.detach(), t, max_wg)
        ctx.t, ctx.max_wg = float(t), int(max_wg)
        ctx.save_for_backward(xc, S)
        return loss.clone()

    @staticmethod
    def backward(ctx, g):
        x, S = ctx.saved_tensors
        return _uniformity_bwd(x, ctx.t, S, g, ctx.max_wg), None, None


class AlignLossFn(Function):
    """``scale * sum over the positives (label == 1) of (2 - 2 z)`` for logits [B, N] and float64 labels, a float64 scalar —
    ``sbr_align_fwd`` / ``sbr_align_bwd``. On cosine logits with ``scale = 1 / B`` it is DirectAU's alignment term
    ``mean_b |u^_b - i^_b|^2``. Negative columns get a zero gradient. Block partials are added in block order in either mode."""

    @staticmethod
    def forward(ctx, logits, labels, scale: float):
        _need_cuda(logits)
        logits = _f32c(logits)
        B, N = logits.shape
        lab = labels.to(device=logits.device, dtype=torch.float64).contiguous()
        if tuple(lab.shape) != (B, N):
            raise ValueError(f'AlignLossFn: labels {tuple(lab.shape)} do not match the logits [{B}, {N}]')
        out = torch.empty((), device=logits.device, dtype=torch.float64)
        call('sbr_align_fwd', ptr(logits), ptr(lab), B, N, float(scale), ptr(out), stream())
        ctx.scale = float(scale)
        ctx.save_for_backward(lab)
        return out

    @staticmethod
    def backward(ctx, g):
        lab, = ctx.saved_tensors
        B, N = lab.shape
        g = g.contiguous()
        d = torch.empty((B, N), device=lab.device, dtype=torch.float32)
        call('sbr_align_bwd', ptr(lab), B, N, ctx.scale, ptr(g), 1 if g.dtype == torch.float64 else 0, ptr(d), stream())
        return d, None, None


# ---- UltraGCN (csrc/ultragcn.hip) --------------------------------------------------------------------------------------------------------
COOC_MAX_K = 64                   # the longest list of sbr_cooc_weight_topk, and the most neighbour slots of the fused loss
ULTRAGCN_MAX_D = 256


def _f32_vec(who, name, t, n):
    if t.dtype != torch.float32 or tuple(t.shape) != (n,) or not t.is_contiguous():
        raise ValueError(f'{who}: {name} must be a contiguous float32 [{n}], got {t.dtype} {tuple(t.shape)}')
    return t


def cooc_weight_topk(csr, row_scale: torch.Tensor, col_scale: torch.Tensor, k: int, include_self: bool = True, rows=None,
                     tile_cols: int = 0):
    """The ``k`` heaviest co-occurrence partners of every COLUMN (item) of a binary resident ``features.DeviceCSR`` X [n, m]: with
    ``G = X^T X`` the value of the pair (i, j), ``G_ij > 0``, is ``(float(G_ij) * row_scale[i]) * col_scale[j]`` in float32
    (``sbr_cooc_weight_topk`` with X^T as its matrix) -> ``(idx int32 [m, k], val float32 [m, k], len int32 [m])``, every list sorted by
    (value descending, index ascending), (-1, 0) behind its length. ``include_self``: item i is a candidate of its own list.
    ``rows=(r0, r1)`` computes that range of items only (the others come back empty): the same bits as the whole. 1 <= k <= 64. Nothing
    of size m x m exists; integer atomics only."""
    _need_cuda(csr.indptr, row_scale, col_scale)
    if csr.data is not None:
        raise ValueError('cooc_weight_topk: co-occurrence counts are stated for 0/1 data; this matrix has values')
    n, m = csr.shape
    dev = csr.indptr.device
    _f32_vec('cooc_weight_topk', 'row_scale', row_scale, m)
    _f32_vec('cooc_weight_topk', 'col_scale', col_scale, m)
    r0, r1, whole = _row_range(rows, m)
    t_indptr, t_indices, _ = csr.transposed()
    idx = (torch.empty if whole else partial(torch.full, fill_value=-1))((m, k), device=dev, dtype=torch.int32)
    val = (torch.empty if whole else torch.zeros)((m, k), device=dev, dtype=torch.float32)
    length = (torch.empty if whole else torch.zeros)((m,), device=dev, dtype=torch.int32)
    # the items are the rows of X^T: X^T is the entry's matrix, X its transpose
    call('sbr_cooc_weight_topk', ptr(t_indptr), ptr(t_indices), ptr(csr.indptr), ptr(csr.indices), m, n, r0, r1, ptr(row_scale), ptr(col_scale),
         1 if include_self else 0, int(k), int(tile_cols), ptr(idx), ptr(val), ptr(length), stream())
    return idx, val, length


def ultragcn_scales(csr):
    """UltraGCN's degree vectors of the binary resident users x items matrix X, on its device, nothing read back:
    ``(beta_u [n_users], beta_i [n_items], row_scale [n_items], col_scale [n_items])`` float32 with ``beta_u = sqrt(d_u + 1) / d_u`` (0 where
    ``d_u = 0``), ``beta_i = 1 / sqrt(d_i + 1)``, ``row_scale = sqrt(g + 1) / g`` (0 where ``g = 0``), ``col_scale = 1 / sqrt(g + 1)`` and
    ``g_i = sum over the users u of item i of d_u``, the row sums of ``X^T X``. The degrees and g are exact integers (row lengths; one
    int64 prefix sum over X^T's entries); each scale is evaluated in float64 and rounded to float32 once."""
    _need_cuda(csr.indptr)
    t_indptr, t_indices, _ = csr.transposed()
    d_u = csr.indptr[1:] - csr.indptr[:-1]
    d_i = t_indptr[1:] - t_indptr[:-1]
    run = torch.zeros(t_indices.numel() + 1, device=d_u.device, dtype=torch.int64)
    run[1:] = torch.cumsum(d_u[t_indices.long()], 0)
    g = run[t_indptr[1:]] - run[t_indptr[:-1]]

    def up(x):                    # sqrt(x + 1) / x, 0 where x = 0
        xd = x.double()
        return torch.where(x > 0, torch.sqrt(xd + 1) / xd.clamp(min=1), torch.zeros_like(xd)).float()

    def down(x):                  # 1 / sqrt(x + 1)
        return (1 / torch.sqrt(x.double() + 1)).float()

    return up(d_u), down(d_i), up(g), down(g)


def _ultragcn_operands(Ub, V, u_idxs, i_idxs, beta_u, beta_i, nbr_idx, nbr_val, nbr_len):
    who = 'UltraGCNLossFn'
    _need_cuda(Ub, V, u_idxs, i_idxs, beta_u, beta_i, nbr_idx, nbr_val, nbr_len)
    if V.dim() != 2 or V.dtype != torch.float32 or not V.is_contiguous():
        raise ValueError(f'{who}: the item table must be a contiguous float32 matrix [n_items, D] (its rows are read in place), got '
                         f'{V.dtype} {tuple(V.shape)} strides {V.stride()}')
    n_items, D = int(V.shape[0]), int(V.shape[1])
    if i_idxs.dim() != 2 or u_idxs.dim() != 1 or u_idxs.shape[0] != i_idxs.shape[0] or tuple(Ub.shape) != (u_idxs.shape[0], D):
        raise ValueError(f'{who}: needs u_idxs [B], i_idxs [B, 1 + N] and Ub [B, {D}], got {tuple(u_idxs.shape)}, {tuple(i_idxs.shape)} and '
                         f'{tuple(Ub.shape)}')
    B, N = int(i_idxs.shape[0]), int(i_idxs.shape[1]) - 1
    if nbr_idx.dim() != 2 or nbr_idx.shape[0] != n_items or nbr_val.shape != nbr_idx.shape or tuple(nbr_len.shape) != (n_items,) \
            or nbr_idx.dtype != torch.int32 or nbr_len.dtype != torch.int32 or nbr_val.dtype != torch.float32 \
            or not (nbr_idx.is_contiguous() and nbr_val.is_contiguous() and nbr_len.is_contiguous()):
        raise ValueError(f'{who}: the neighbour lists must be contiguous (int32 [{n_items}, K], float32 [{n_items}, K], int32 [{n_items}])')
    _f32_vec(who, 'beta_i', beta_i, n_items)
    _f32_vec(who, 'beta_u', beta_u, beta_u.shape[0] if beta_u.dim() == 1 else -1)
    return (_f32c(Ub), V, u_idxs.to(torch.int32).contiguous(), i_idxs.to(torch.int32).contiguous(), B, D, N, int(nbr_idx.shape[1]),
            int(beta_u.shape[0]), n_items)


class UltraGCNLossFn(Function):
    """UltraGCN's objective on a batch (Mao et al., CIKM 2021) -> ``(loss, parts [3], scores [B, 1 + N])``: ``loss = pos +
    negative_weight * neg + lam * nbr`` summed over the batch, ``parts = (pos, neg, nbr)`` and the dot products of the sampled slots, the
    last two without a gradient. ``Ub`` [B, D]: the users' rows (``LookupFn``: the user table's gradient takes the existing path); ``V``
    [n_items, D]: the item table itself, contiguous, read in place; ``i_idxs`` [B, 1 + N] with the positive in column 0; ``beta_u`` /
    ``beta_i`` and the lists of ``cooc_weight_topk`` as in include/sibrar_hip.h. The forward pass is one call of
    ``sbr_ultragcn_loss_fwd_bwd``, which also leaves dL/dUb and the coefficients dL/ds [B, 1 + N + K]; no [B, 1 + N + K, D] copy of item
    rows or of their gradient exists. The backward pass scales dL/dUb and gathers the item table's gradient from the coefficients
    (``sbr_scatter_add_scaled_rows_sorted`` behind a stable sort of the slots' item indices, padded slots under a sentinel key; the
    upstream scalar is read on the device). Fixed order, no atomics: the only form, valid in deterministic mode. 1 <= D <= 256, N >= 1,
    1 <= K <= 64."""

    @staticmethod
    def forward(ctx, Ub, V, u_idxs, i_idxs, beta_u, beta_i, nbr_idx, nbr_val, nbr_len, w1, w2, w3, w4, negative_weight, lam):
        Ub, V, u32, i32, B, D, N, K, n_users, n_items = _ultragcn_operands(Ub.detach(), V.detach(), u_idxs, i_idxs, beta_u, beta_i, nbr_idx,
                                                                            nbr_val, nbr_len)
        dev = V.device
        parts = torch.empty(4, device=dev, dtype=torch.float32)
        dUb = torch.empty(B, D, device=dev, dtype=torch.float32)
        coef = torch.empty(B, 1 + max(N, 0) + K, device=dev, dtype=torch.float32)
        scores = torch.empty(B, 1 + max(N, 0), device=dev, dtype=torch.float32)
        ws, ws_bytes = _entry_ws(dev, 'sbr_ultragcn_loss', B, dtype=torch.float64)
        call('sbr_ultragcn_loss_fwd_bwd', ptr(Ub), ptr(V), ptr(u32), ptr(i32), ptr(beta_u), ptr(beta_i), ptr(nbr_idx), ptr(nbr_val),
             ptr(nbr_len), B, D, N, K, n_users, n_items, float(w1), float(w2), float(w3), float(w4), float(negative_weight), float(lam),
             ptr(parts), ptr(dUb), ptr(coef), ptr(scores), ws, ws_bytes, stream())
        ctx.save_for_backward(Ub, dUb, coef, i32, nbr_idx)
        ctx.v_shape = (n_items, D)
        loss, three = parts[3].clone(), parts[:3].clone()
        ctx.mark_non_differentiable(three, scores)
        return loss, three, scores

    @staticmethod
    def backward(ctx, g, _g_parts, _g_scores):
        Ub, dUb, coef, i32, nbr_idx = ctx.saved_tensors
        n_items, D = ctx.v_shape
        g = g.reshape(1).to(torch.float32).contiguous()
        d_ub = dUb * g if ctx.needs_input_grad[0] else None
        dV = None
        if ctx.needs_input_grad[1]:
            dV = torch.zeros(n_items, D, device=coef.device, dtype=torch.float32)
            if coef.numel() > 0:
                # the slots' keys: the item each slot names; padded neighbour slots (-1) and indices outside the table take the sentinel
                p = i32[:, 0].long().clamp(0, max(n_items - 1, 0))
                keys = torch.cat([i32, nbr_idx[p]], dim=1).reshape(-1)
                keys = torch.where((keys < 0) | (keys >= n_items), torch.full_like(keys, n_items), keys)
                skeys, order = torch.sort(keys, stable=True)
                call('sbr_scatter_add_scaled_rows_sorted', ptr(coef), ptr(Ub), ptr(skeys), ptr(order), keys.numel(), coef.shape[1], ptr(g),
                     ptr(dV), n_items, D, stream())
        return (d_ub, dV) + (None,) * 13


# ---- SimpleX (csrc/simplex.hip) -----------------------------------------------------------------------------------------------------------
CCL_MAX_D = 256


def _ccl_operands(H, V, i_idxs):
    who = 'CCLLossFn'
    _need_cuda(H, V, i_idxs)
    if V.dim() != 2 or V.dtype != torch.float32 or not V.is_contiguous():
        raise ValueError(f'{who}: the item table must be a contiguous float32 matrix [n_items, D] (its rows are read in place), got '
                         f'{V.dtype} {tuple(V.shape)} strides {V.stride()}')
    n_items, D = int(V.shape[0]), int(V.shape[1])
    if i_idxs.dim() != 2 or H.dim() != 2 or tuple(H.shape) != (i_idxs.shape[0], D):
        raise ValueError(f'{who}: needs i_idxs [B, 1 + N] and H [B, {D}], got {tuple(i_idxs.shape)} and {tuple(H.shape)}')
    return _f32c(H), V, i_idxs.to(torch.int32).contiguous(), int(i_idxs.shape[0]), D, int(i_idxs.shape[1]) - 1, n_items


class CCLLossFn(Function):
    """SimpleX's cosine contrastive loss on a batch (Mao et al., CIKM 2021) -> ``(loss, parts [2], scores [B, 1 + N])``: with ``y`` the
    cosine of ``H[b]`` and an item row (norms clamped at ``COS_EPS``), ``loss = mean_b ((1 - y(b, p)) + (negative_weight / N) sum_c
    max(0, y(b, j_c) - margin))``, ``parts = (mean positive term, mean negative term)`` and the cosines of the sampled slots, the last
    two without a gradient. ``H`` [B, D]: the user representations; ``V`` [n_items, D]: the item table itself, contiguous, read in
    place; ``i_idxs`` [B, 1 + N] with the positive in column 0. The forward pass is one call of ``sbr_ccl_loss_fwd_bwd``, which also
    leaves dL/dH and the two coefficient arrays [B, 1 + N] of the item table's gradient (include/sibrar_hip.h); no [B, 1 + N, D] copy
    of item rows or of their gradient exists. The backward pass scales dL/dH and gathers the item table's gradient from the
    coefficients (``sbr_scatter_add_cos_rows_sorted`` behind a stable sort of the slots' item indices, indices outside the table under
    a sentinel key; the upstream scalar is read on the device). Fixed order, no atomics: the only form, valid in deterministic mode.
    1 <= D <= 256, N >= 1."""

    @staticmethod
    def forward(ctx, H, V, i_idxs, margin, negative_weight):
        H, V, i32, B, D, N, n_items = _ccl_operands(H.detach(), V.detach(), i_idxs)
        dev = V.device
        parts = torch.empty(3, device=dev, dtype=torch.float32)
        dH = torch.empty(B, D, device=dev, dtype=torch.float32)
        coef_a = torch.empty(B, 1 + max(N, 0), device=dev, dtype=torch.float32)
        coef_s = torch.empty_like(coef_a)
        scores = torch.empty_like(coef_a)
        ws, ws_bytes = _entry_ws(dev, 'sbr_ccl_loss', B, dtype=torch.float64)
        call('sbr_ccl_loss_fwd_bwd', ptr(H), ptr(V), ptr(i32), B, D, N, n_items, float(margin), float(negative_weight), COS_EPS, ptr(parts),
             ptr(dH), ptr(coef_a), ptr(coef_s), ptr(scores), ws, ws_bytes, stream())
        ctx.save_for_backward(H, V, dH, coef_a, coef_s, i32)
        loss, two = parts[2].clone(), parts[:2].clone()
        ctx.mark_non_differentiable(two, scores)
        return loss, two, scores

    @staticmethod
    def backward(ctx, g, _g_parts, _g_scores):
        H, V, dH, coef_a, coef_s, i32 = ctx.saved_tensors
        n_items, D = V.shape
        g = g.reshape(1).to(torch.float32).contiguous()
        d_h = dH * g if ctx.needs_input_grad[0] else None
        dV = None
        if ctx.needs_input_grad[1]:
            dV = torch.zeros(n_items, D, device=V.device, dtype=torch.float32)
            if coef_a.numel() > 0:
                keys = i32.reshape(-1)                            # the item each slot names; indices outside the table take the sentinel
                keys = torch.where((keys < 0) | (keys >= n_items), torch.full_like(keys, n_items), keys)
                skeys, order = torch.sort(keys, stable=True)
                call('sbr_scatter_add_cos_rows_sorted', ptr(coef_a), ptr(coef_s), ptr(H), ptr(V), ptr(skeys), ptr(order), keys.numel(),
                     coef_a.shape[1], ptr(g), ptr(dV), n_items, D, stream())
        return d_h, dV, None, None, None


# ---- NeuMF (csrc/neumf.hip) -----------------------------------------------------------------------------------------------------------
NEUMF_MAX_H = 64                  # the widest MLP layer (NEUMF_MAX_H in neumf.hip)
NEUMF_MAX_LAYERS = 4              # H1 .. H4 (NEUMF_MAX_LAYERS in neumf.hip)


def neumf_tail_len(widths) -> int:
    """floats of the packed tail for the layer widths (H1, ..., HL): W_2 .. W_L, b_2 .. b_L, w_h, c"""
    return sum(widths[l] * widths[l - 1] + widths[l] for l in range(1, len(widths))) + widths[-1] + 1


def neumf_pack_tail(weights, biases, w_h, c) -> torch.Tensor:
    """One float32 buffer ``[W_2 .. W_L | b_2 .. b_L | w_h | c]`` (each ``W_l`` [H_l, H_{l-1}] row-major) for ``neumf_score_all``: a model
    builds it once per evaluation, not once per user chunk."""
    parts = [w.detach().reshape(-1) for w in weights] + [b.detach().reshape(-1) for b in biases] + [w_h.detach().reshape(-1),
                                                                                                      c.detach().reshape(-1)]
    return torch.cat([p.to(torch.float32) for p in parts]).contiguous()


def _neumf_widths(who, widths, tail):
    widths = tuple(int(w) for w in widths)
    if not 1 <= len(widths) <= NEUMF_MAX_LAYERS:
        raise ValueError(f'{who}: {len(widths)} layer widths outside [1, {NEUMF_MAX_LAYERS}]')
    if any(not 1 <= w <= NEUMF_MAX_H for w in widths):
        raise ValueError(f'{who}: layer widths {widths} outside [1, {NEUMF_MAX_H}]')
    if tail.dim() != 1 or tail.dtype != torch.float32 or not tail.is_contiguous() or tail.numel() != neumf_tail_len(widths):
        raise ValueError(f'{who}: the packed tail must be a contiguous float32 vector of {neumf_tail_len(widths)} elements for the widths '
                         f'{widths} (ops.neumf_pack_tail), got {tail.dtype} {tuple(tail.shape)}')
    return widths + (0,) * (NEUMF_MAX_LAYERS - len(widths))


def _neumf_rows(who, name, t, h1):
    """-> the row stride of the float32 matrix ``t`` [n, h1], whose rows are contiguous and may lie any distance apart"""
    if t.dim() != 2 or t.dtype != torch.float32 or t.shape[1] != h1:
        raise ValueError(f'{who}: {name} must be a float32 matrix [n, {h1}], got {t.dtype} {tuple(t.shape)}')
    if (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError(f'{who}: the rows of {name} must be contiguous and apart by at least their length, got strides {t.stride()}')
    return max(int(t.stride(0)), int(t.shape[1])) if t.shape[0] > 1 else int(t.shape[1])


def neumf_score_all(A: torch.Tensor, Bt: torch.Tensor, tail: torch.Tensor, widths, out: Optional[torch.Tensor] = None,
                    accumulate: bool = False) -> torch.Tensor:
    """NeuMF's MLP term of every user against every item without the [Bu, I, H1] activation (``sbr_neumf_score_all``), no autograd:
    ``out[u, i] = <w_h, z_L> + c`` with ``z_1 = relu(A[u] + Bt[i])`` and ``z_l = relu(W_l z_{l-1} + b_l)``. ``A`` [Bu, H1] is the user
    half of the first layer with its bias, ``Bt`` [I, H1] the item half; ``tail`` is ``neumf_pack_tail`` for ``widths`` = (H1, ..., HL).
    All three matrices are float32 with contiguous rows at any row stride. ``accumulate``: add onto ``out`` (the GMF term, laid down by
    the fp32 GEMM) instead of overwriting it. A pair's bits do not depend on how users are chunked or items sharded."""
    who = 'neumf_score_all'
    _need_cuda(A, Bt, tail, out)
    h = _neumf_widths(who, widths, tail)
    lda, ldb = _neumf_rows(who, 'A', A, h[0]), _neumf_rows(who, 'Bt', Bt, h[0])
    Bu, I = int(A.shape[0]), int(Bt.shape[0])
    if out is None:
        if accumulate:
            raise ValueError(f'{who}: accumulate=True adds onto out, which is missing')
        out = torch.empty(Bu, I, device=A.device, dtype=torch.float32)
    if tuple(out.shape) != (Bu, I):
        raise ValueError(f'{who}: out must be [{Bu}, {I}], got {tuple(out.shape)}')
    ldo = _neumf_rows(who, 'out', out, I)
    if Bu == 0 or I == 0:
        return out
    call('sbr_neumf_score_all', ptr(A), lda, ptr(Bt), ldb, ptr(tail), tail.numel(), len(tuple(widths)), *h, ptr(out), ldo, Bu, I,
         1 if accumulate else 0, stream())
    return out


def neumf_score_pairs(A: torch.Tensor, Bt: torch.Tensor, u_slot: torch.Tensor, i_slot: torch.Tensor, tail: torch.Tensor, widths,
                      out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """The score of ``neumf_score_all`` for the listed pairs (``sbr_neumf_score_pairs``): ``out[r]`` is the pair (row ``u_slot[r]`` of
    ``A``, row ``i_slot[r]`` of ``Bt``), bit for bit what ``neumf_score_all`` gives that pair. A slot outside its matrix gives a NaN."""
    who = 'neumf_score_pairs'
    _need_cuda(A, Bt, tail, u_slot, i_slot, out)
    h = _neumf_widths(who, widths, tail)
    lda, ldb = _neumf_rows(who, 'A', A, h[0]), _neumf_rows(who, 'Bt', Bt, h[0])
    if u_slot.dim() != 1 or u_slot.shape != i_slot.shape:
        raise ValueError(f'{who}: u_slot and i_slot must be vectors of one length, got {tuple(u_slot.shape)} and {tuple(i_slot.shape)}')
    R = int(u_slot.numel())
    if out is None:
        if accumulate:
            raise ValueError(f'{who}: accumulate=True adds onto out, which is missing')
        out = torch.empty(R, device=A.device, dtype=torch.float32)
    if tuple(out.shape) != (R,) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f'{who}: out must be a contiguous float32 vector [{R}], got {out.dtype} {tuple(out.shape)}')
    if R == 0:
        return out
    u32, i32 = u_slot.to(torch.int32).contiguous(), i_slot.to(torch.int32).contiguous()
    call('sbr_neumf_score_pairs', ptr(A), lda, int(A.shape[0]), ptr(Bt), ldb, int(Bt.shape[0]), ptr(u32), ptr(i32), ptr(tail),
         tail.numel(), len(tuple(widths)), *h, ptr(out), R, 1 if accumulate else 0, stream())
    return out


# ---- implicit-feedback ALS (csrc/als.hip) -------------------------------------------------------------------------------------------
def als_gram(Y: torch.Tensor, reg: float) -> torch.Tensor:
    """``Y^T Y + reg I`` as float32 [f, f] for the factor matrix ``Y`` [n, f], f <= 128: the part of the ALS system every row of a
    half-sweep shares (``sbr_als_gram_f32``: row slabs added in slab order, the same bits on every run)."""
    _need_cuda(Y)
    n, f, ldy = _f32_rows_view('als_gram', 'Y', Y)
    G = torch.empty(f, f, device=Y.device, dtype=torch.float32)
    call('sbr_als_gram_f32', ptr(Y), n, ldy, f, float(reg), ptr(G), max(f, 1), *_entry_ws(Y.device, 'sbr_als_gram_f32', n, f), stream())
    return G


def als_solve_rows(csr, Y: torch.Tensor, G: torch.Tensor, alpha: float, out=None, rows=None) -> torch.Tensor:
    """One ALS half-sweep over the rows ``rows=(r0, r1)`` (None: every row) of the resident ``features.DeviceCSR`` ``csr`` [n, n_y]:
    ``out[r] = (G + sum_i (alpha r_i - 1) y_i y_i^T)^-1 sum_i alpha r_i y_i`` over the entries i of row r, with ``G = als_gram(Y, reg)``
    (``sbr_als_solve_rows_f32``: one workgroup per row, Cholesky in LDS). ``out``: a float32 [n, f] view with unit column stride to
    write into (the rows outside the range keep what they hold; those of a new result are zero). Raises ``SibrarHipError`` naming the
    first row whose system is not positive definite in float32. Reads one int32 back: synchronises with the stream."""
    _need_cuda(csr.indptr, Y, G, out)
    n, n_y = csr.shape
    ny, f, ldy = _f32_rows_view('als_solve_rows', 'Y', Y)
    if ny != n_y:
        raise ValueError(f'als_solve_rows: Y has {ny} rows, the matrix {n_y} columns')
    if G.dtype != torch.float32 or tuple(G.shape) != (f, f):
        raise ValueError(f'als_solve_rows: G must be float32 [{f}, {f}], got {G.dtype} {tuple(G.shape)}')
    G = G.contiguous()
    r0, r1, whole = _row_range(rows, n, 'als_solve_rows')
    out, ldo = _rows_out('als_solve_rows', out, (n, f), whole, Y.device)
    info = torch.zeros(1, device=Y.device, dtype=torch.int32)
    call('sbr_als_solve_rows_f32', ptr(csr.indptr), ptr(csr.indices), ptr(csr.data), r0, r1, ptr(Y), n_y, ldy, f, ptr(G), float(alpha),
         ptr(out), ldo, ptr(info), stream())
    _check_info(info, lambda bad: SibrarHipError(
        f'als_solve_rows: the system of row {bad - 1} is not positive definite in float32 (a pivot of its Cholesky factorisation is not '
        f'positive); the fp32 factorisation needs `regularization` well above f * 2^-24 * ||A|| (f = {f}, alpha = {float(alpha):g}): raise '
        f'`regularization` or lower `factors`'))
    return out


# ---- truncated SVD by block subspace iteration (csrc/svd.hip) -----------------------------------------------------------------------
def gram(Y: torch.Tensor) -> torch.Tensor:
    """``Y^T Y`` as float32 [f, f] for ``Y`` [n, f], f <= 128 (``sbr_gram_f32``: ``als_gram``'s kernels with nothing added to the
    diagonal; symmetric bit for bit, the same bits on every run)."""
    _need_cuda(Y)
    n, f, ldy = _f32_rows_view('gram', 'Y', Y)
    _block_width('gram', f)
    G = torch.empty(f, f, device=Y.device, dtype=torch.float32)
    call('sbr_gram_f32', ptr(Y), n, ldy, f, ptr(G), f, *_entry_ws(Y.device, 'sbr_als_gram_f32', n, f), stream())
    return G


def sym_eig(A: torch.Tensor, info: Optional[torch.Tensor] = None):
    """``(lam [n] descending, W [n, n])`` with ``A = W diag(lam) W^T`` for a symmetric float32 ``A`` [n, n] (a square row-major view,
    its lower triangle is read), 1 <= n <= 128, by the one-workgroup Jacobi of ``sbr_sym_eig_f32`` (iterated in double, rounded once); every eigenvector's component of
    largest magnitude is positive. The same bits on every run. Raises ``SibrarHipError`` when the sweep cap was reached with rotations
    still happening. ``info``: the device int32 [1] the kernel reports into instead of a fresh zero (tests: a word that is set on entry
    stands for a run that did not converge). Reads one int32 back: synchronises with the stream."""
    _need_cuda(A, info)
    n, _, lda = _f32_rows_view('sym_eig', 'A', A, square=True)
    _block_width('sym_eig', n)
    if info is None:
        info = torch.zeros(1, device=A.device, dtype=torch.int32)
    elif info.dtype != torch.int32 or info.numel() != 1:
        raise ValueError(f'sym_eig: info must be one int32, got {info.dtype} {tuple(info.shape)}')
    W = torch.empty(n, n, device=A.device, dtype=torch.float32)
    lam = torch.empty(n, device=A.device, dtype=torch.float32)
    call('sbr_sym_eig_f32', ptr(A), n, lda, ptr(W), n, ptr(lam), ptr(info), *_entry_ws(A.device, 'sbr_sym_eig_f32', n, dtype=torch.float64),
         stream())
    _check_info(info, lambda bad: SibrarHipError(
        f'sym_eig: the Jacobi iteration on the [{n}, {n}] matrix still rotated in sweep {bad - 1}, its last (info = {bad}): the matrix holds '
        f'non-finite values, or is no symmetric matrix of float32 numbers'))
    return lam, W


def csr_times_dense(csr, D: torch.Tensor, out=None, rows=None) -> torch.Tensor:
    """``X @ D`` as float32 [n, c] for the resident ``features.DeviceCSR`` (or a namespace with ``shape``, ``indptr``, ``indices``,
    ``data``) X [n, n_d] and ``D`` [n_d, c], c <= 128, over the rows ``rows=(r0, r1)`` (None: every row) — ``sbr_csr_times_dense_f32``:
    one fmaf chain per element in ascending CSR order, the same bits for every split of the rows. ``out``: a float32 [n, c] view with
    unit column stride to write into (the rows outside the range keep what they hold; those of a new result are zero)."""
    _need_cuda(csr.indptr, D, out)
    n, n_d = csr.shape
    nd, c, ldd = _f32_rows_view('csr_times_dense', 'D', D)
    if nd != n_d:
        raise ValueError(f'csr_times_dense: D has {nd} rows, the matrix {n_d} columns')
    _block_width('csr_times_dense', c)
    r0, r1, whole = _row_range(rows, n, 'csr_times_dense')
    out, ldo = _rows_out('csr_times_dense', out, (n, c), whole, D.device)
    call('sbr_csr_times_dense_f32', ptr(csr.indptr), ptr(csr.indices), ptr(csr.data), r0, r1, ptr(D), n_d, ldd, c, ptr(out), ldo, stream())
    return out


def rotate_cols(Y: torch.Tensor, W: torch.Tensor, lam: Optional[torch.Tensor] = None, out=None):
    """``Y W diag(1 / s)`` with ``s = sqrt(max(lam, tiny))`` -> ``(out [n, b], s [b])``, or the plain ``Y W`` -> ``out`` when ``lam``
    is None (``sbr_rotate_cols_f32``: an fp32 fmaf chain per element in ascending k). ``Y`` [n, b] and ``out`` are float32 views with
    unit column stride; ``out`` may be ``Y`` itself. ``W`` float32 [b, b], ``lam`` float32 [b], as ``sym_eig`` returns them."""
    _need_cuda(Y, W, lam, out)
    n, b, ldy = _f32_rows_view('rotate_cols', 'Y', Y)
    _block_width('rotate_cols', b)
    ldw = _f32_rows_view('rotate_cols', 'W', W, (b, b))[2]
    if lam is not None and (lam.dtype != torch.float32 or tuple(lam.shape) != (b,) or not lam.is_contiguous()):
        raise ValueError(f'rotate_cols: lam must be a contiguous float32 [{b}], got {lam.dtype} {tuple(lam.shape)}')
    out, ldo = _rows_out('rotate_cols', out, (n, b), True, Y.device)
    s = None if lam is None else torch.empty(b, device=Y.device, dtype=torch.float32)
    call('sbr_rotate_cols_f32', ptr(Y), n, ldy, b, ptr(W), ldw, ptr(lam), ptr(s), ptr(out), ldo, stream())
    return out if lam is None else (out, s)


def col_residual(Y: torch.Tensor, U: torch.Tensor, s: torch.Tensor, f: int) -> torch.Tensor:
    """``||Y[:, j] - s[j] U[:, j]||_2`` for j < f as float32 [f] (``sbr_col_residual_f32``, fixed order); ``Y`` and ``U`` float32
    [n, >= f] views with unit column stride, ``s`` a contiguous float32 vector of at least f elements."""
    _need_cuda(Y, U, s)
    n, cy, ldy = _f32_rows_view('col_residual', 'Y', Y)
    nu, cu, ldu = _f32_rows_view('col_residual', 'U', U)
    _block_width('col_residual', f)
    if nu != n or f > min(cy, cu) or s.dtype != torch.float32 or s.dim() != 1 or s.numel() < f or not s.is_contiguous():
        raise ValueError(f'col_residual: f={f} columns of Y {tuple(Y.shape)}, U {tuple(U.shape)} and s {s.dtype} {tuple(s.shape)} are asked for')
    res = torch.empty(f, device=Y.device, dtype=torch.float32)
    call('sbr_col_residual_f32', ptr(Y), ldy, ptr(U), ldu, ptr(s), n, f, ptr(res), *_entry_ws(Y.device, 'sbr_col_residual_f32', n, f), stream())
    return res


# ---- RBMF: representative rows by maxvol, and the ridge solve (csrc/rbmf.hip) -------------------------------------------------------------
MAXVOL_GROUP = 16                 # swap launches enqueued between two read-backs of the swap counter


def tri_solve_rows(X: torch.Tensor, T: torch.Tensor, upper: bool = False, unit: bool = False, out=None) -> torch.Tensor:
    """``X T^-1`` row by row for ``X`` float32 [n, r] and a triangular ``T`` float32 [r, r], r <= 128 (``sbr_tri_solve_rows_f32``: T in
    LDS, a wave per row, one fmaf chain per element). ``upper``: which triangle of ``T`` is read; ``unit``: its diagonal is taken as 1.
    ``X``, ``T`` and ``out`` are views with unit column stride; ``out`` may be ``X`` itself."""
    _need_cuda(X, T, out)
    n, r, ldx = _f32_rows_view('tri_solve_rows', 'X', X)
    _block_width('tri_solve_rows', r)
    ldt = _f32_rows_view('tri_solve_rows', 'T', T, (r, r))[2]
    out, ldo = _rows_out('tri_solve_rows', out, (n, r), True, X.device)
    call('sbr_tri_solve_rows_f32', ptr(X), ldx, n, r, ptr(T), ldt, int(bool(upper)), int(bool(unit)), ptr(out), ldo, stream())
    return out


def cholesky(K: torch.Tensor) -> torch.Tensor:
    """The lower triangular ``R`` float32 [n, n] with ``K = R R^T`` for a symmetric positive definite float32 ``K`` (a square row-major
    view whose lower triangle is read), n <= 128 — ``sbr_chol_f32``, the LDS factorisation of ``als_solve_rows``. Raises
    ``SibrarHipError`` naming the first pivot that is not positive in float32. Reads one int32 back: synchronises with the stream."""
    _need_cuda(K)
    n, _, ldk = _f32_rows_view('cholesky', 'K', K, square=True)
    _block_width('cholesky', n)
    R = torch.empty(n, n, device=K.device, dtype=torch.float32)
    info = torch.zeros(1, device=K.device, dtype=torch.int32)
    call('sbr_chol_f32', ptr(K), n, ldk, ptr(R), n, ptr(info), stream())
    _check_info(info, lambda bad: SibrarHipError(
        f'cholesky: the [{n}, {n}] matrix is not positive definite in float32 (pivot {bad - 1} of its Cholesky factorisation is not '
        f'positive): raise the ridge term well above n * 2^-24 * ||K||'))
    return R


def _maxvol_ws(device, n, slab_rows):
    ws = _entry_ws(device, 'sbr_maxvol_f32', n, int(slab_rows), dtype=torch.int32)
    if not ws[1]:
        raise ValueError(f'maxvol: slab_rows={slab_rows} outside [0, 1024] (n = {n})')
    return ws


def maxvol_lu(A: torch.Tensor, slab_rows: int = 0, want_upper: bool = False):
    """The row-pivoted LU of ``A`` float32 [n, r] (n >= r, r <= 128), IN PLACE, by r launches of ``sbr_maxvol_lu_step_f32`` with no
    read-back in between -> ``(idx int32 [r], L_top [r, r], U_top [r, r] or None)``: the pivot rows in pivot order, ``A`` overwritten
    with the unit lower factor over all rows, its pivot rows, and (``want_upper``) the upper factor: ``A_in[idx] = L_top U_top``. Raises
    ``SibrarHipError`` naming the first step whose pivot is not above r * 2^-24 * the largest pivot before it: the block has numerical
    rank below r. Reads one int32 back: synchronises with the stream."""
    _need_cuda(A)
    n, r, lda = _f32_rows_view('maxvol_lu', 'A', A)
    _block_width('maxvol_lu', r, n)
    ws = _maxvol_ws(A.device, n, slab_rows)
    idx = torch.empty(r, device=A.device, dtype=torch.int32)
    ltop = torch.empty(r, r, device=A.device, dtype=torch.float32)
    utop = torch.empty(r, r, device=A.device, dtype=torch.float32) if want_upper else None
    info = torch.zeros(1, device=A.device, dtype=torch.int32)
    for k in range(r):
        call('sbr_maxvol_lu_step_f32', ptr(A), n, lda, r, k, ptr(idx), ptr(ltop), r, ptr(utop), r, ptr(info), *ws, int(slab_rows), stream())
    _check_info(info, lambda bad: SibrarHipError(
        f'maxvol_lu: the pivot of step {bad - 1} of the row-pivoted LU of the [{n}, {r}] block is not above r * 2^-24 * the largest pivot '
        f'before it (or is not finite): the block has numerical rank below {r} in float32; ask for fewer representatives'))
    return idx, ltop, utop


def _maxvol_basis(U, idx, slab_rows):
    """``U inv(U[idx])`` from ``idx`` alone: G = U[idx] = P^T L_top U_top by the LU of the r gathered rows, two triangular solves, and
    the columns put back in basis order (Y[idx[piv[s]]] = e_s, and row idx[c] of the result has to be e_c)"""
    G = U[idx.long()].contiguous()
    piv, gl, gu = maxvol_lu(G, slab_rows, want_upper=True)
    Y = tri_solve_rows(tri_solve_rows(U, gu, upper=True, unit=False), gl, upper=False, unit=True)
    B = torch.empty_like(Y)
    B[:, piv.long()] = Y
    return B


def maxvol(U: torch.Tensor, tol: float = 1.05, max_iters: int = 100, slab_rows: int = 0, start=None):
    """``maxvolpy.maxvol.maxvol(U)`` (algorithms/mf_algs.py:177) for ``U`` float32 [n, r], n >= r, r <= 128 -> ``(idx int64 [r],
    n_swaps)``: r rows whose r x r submatrix has locally maximal volume, ``max |U inv(U[idx])| <= tol`` unless ``max_iters`` swaps were
    not enough. The start is the pivot rows of a row-pivoted LU (``maxvol_lu``), ``B = L L_top^-1`` (``tri_solve_rows``), then
    ``sbr_maxvol_swap_step_f32`` in groups of ``MAXVOL_GROUP`` launches, the swap counter read back once per group. When a chain has
    stopped after swaps, B is computed afresh from ``idx`` (an LU of the r gathered rows, two triangular solves) and the chain goes on
    if the fresh maximum is still above ``tol``. ``U`` is not written. The same bits, and the same ``idx``, on every run and for every
    ``slab_rows`` (0: the default of the header). ``start``: r distinct row indices to start from instead of the LU's pivots (tests)."""
    _need_cuda(U)
    n, r, _ = _f32_rows_view('maxvol', 'U', U)
    _block_width('maxvol', r, n)
    if not (tol >= 1 and tol < float('inf')):
        raise ValueError(f'maxvol: tol ({tol}) has to be a finite number >= 1')
    if int(max_iters) != max_iters or max_iters < 0:
        raise ValueError(f'maxvol: max_iters ({max_iters}) has to be a non-negative integer')
    if start is None:
        B = U.clone(memory_format=torch.contiguous_format)
        idx, ltop, _ = maxvol_lu(B, slab_rows)
        tri_solve_rows(B, ltop, upper=False, unit=True, out=B)
    else:
        idx = torch.as_tensor(start).to(device=U.device, dtype=torch.int32).contiguous()
        if tuple(idx.shape) != (r,) or len(set(idx.tolist())) != r or not 0 <= int(idx.min()) <= int(idx.max()) < n:
            raise ValueError(f'maxvol: start must be {r} distinct rows below {n}')
        B = _maxvol_basis(U, idx, slab_rows)
    ws = _maxvol_ws(U.device, n, slab_rows)
    counter = torch.zeros(1, device=U.device, dtype=torch.int32)
    done, fresh = 0, True                                            # swaps so far; B was computed from idx and has seen no swap since
    while done < max_iters:
        group = min(MAXVOL_GROUP, int(max_iters) - done)
        for s in range(group):
            call('sbr_maxvol_swap_step_f32', ptr(B), n, r, r, float(tol), s, ptr(idx), ptr(counter), *ws, int(slab_rows), stream())
        now = int(counter.item())
        idle, fresh, done = now - done < group, fresh and now == done, now
        if not idle:
            continue                                                 # every launch of the group swapped: the chain may have more to do
        if fresh:
            break                                                    # a B fresh from idx holds nothing above tol
        B, fresh = _maxvol_basis(U, idx, slab_rows), True           # drift: B again from idx alone
    return idx.long(), done


class BiasScoreFn(Function):
    """out[b, n] = base[b, n] + user_bias[u[b]] + item_bias[i[b, n]] + global_bias (sgd_alg.py:186-194, 110-119); every term
    optional (None). Bias tables are 1-D float views of the [n, 1] embedding weights. u None: row b; i None: column n."""

    @staticmethod
    def forward(ctx, base, ub, ib, gb, u, i, B, N):
        dev = next(t for t in (base, ub, ib, gb) if t is not None).device
        base_c = _f32c(base) if base is not None else None
        u_c = u.long().contiguous() if u is not None else None
        i_c = i.long().contiguous() if i is not None else None
        out = torch.empty(B, N, device=dev, dtype=torch.float32)
        call('sbr_bias_score_add_fwd', ptr(ub), ptr(ib), ptr(gb), ptr(u_c), ptr(i_c), ptr(base_c), ptr(out), B, N, stream())
        ctx.save_for_backward(u_c, i_c)
        ctx.shapes = (None if ub is None else ub.shape, None if ib is None else ib.shape, gb is not None, base is not None, B, N)
        return out

    @staticmethod
    def backward(ctx, g):
        u_c, i_c = ctx.saved_tensors
        ub_s, ib_s, has_gb, has_base, B, N = ctx.shapes
        g = _f32c(g)
        need = ctx.needs_input_grad
        d_ub = torch.zeros(ub_s, device=g.device, dtype=torch.float32) if ub_s is not None and need[1] else None
        d_ib = torch.zeros(ib_s, device=g.device, dtype=torch.float32) if ib_s is not None and need[2] else None
        d_gb = torch.zeros(1, device=g.device, dtype=torch.float32) if has_gb and need[3] else None
        if d_ub is not None or d_ib is not None or d_gb is not None:
            call('sbr_bias_score_bwd', ptr(g), ptr(u_c), ptr(i_c), ptr(d_ub), ptr(d_ib), ptr(d_gb), B, N, stream())
        return (g if has_base and need[0] else None), d_ub, d_ib, d_gb, None, None, None, None


class ScoreAllFn(Function):
    """einsum('be,ce->bc') — sgd_alg.py:2109: all users of the batch against all item representations."""

    @staticmethod
    def forward(ctx, u, i):
        _need_cuda(u, i)
        u, i = _f32c(u), _f32c(i)
        ctx.save_for_backward(u, i)
        return linear_nt(u, i)

    @staticmethod
    def backward(ctx, g):
        u, i = ctx.saved_tensors
        g = _f32c(g)
        du = matmul_nn(g, i) if ctx.needs_input_grad[0] else None
        di = matmul_tn(g, u) if ctx.needs_input_grad[1] else None
        return du, di


def score(u_repr: torch.Tensor, i_repr: torch.Tensor) -> torch.Tensor:
    """The dot-product score of every model: the item side is [B, N, E] in training (``ScoreDotFn``: one dot per slot) and a matrix
    [I, E] in evaluation (``ScoreAllFn``: all pairs, eval/eval.py:209-217)."""
    return (ScoreAllFn if i_repr.ndim == 2 else ScoreDotFn).apply(u_repr, i_repr)


# ---- losses -------------------------------------------------------------------------------------------------------------------
LOSS_CODES = {'bce': 0, 'bpr': 1, 'sampled_softmax': 2}


class RecLossFn(Function):
    """train/rec_losses.py:43-113. Returns a float64 scalar for bce / bpr (float64 labels promote the computation in the
    reference) and a float32 scalar for sampled softmax."""

    @staticmethod
    def forward(ctx, logits, labels, kind: int, scale: float, shift: float):
        _need_cuda(logits)
        logits = _f32c(logits)
        B, N = logits.shape
        lab = None
        if kind != 2:
            lab = labels.to(device=logits.device, dtype=torch.float64).contiguous()
        out = torch.empty((), device=logits.device, dtype=torch.float64)
        call('sbr_rec_loss_fwd', kind, ptr(logits), ptr(lab), B, N, scale, shift, ptr(out), stream())
        ctx.args = (kind, scale, shift)
        ctx.save_for_backward(logits, lab if lab is not None else torch.empty(0, device=logits.device))
        return out if kind != 2 else out.float()

    @staticmethod
    def backward(ctx, g):
        logits, lab = ctx.saved_tensors
        kind, scale, shift = ctx.args
        B, N = logits.shape
        g = g.contiguous()
        d = torch.empty_like(logits)
        call('sbr_rec_loss_bwd', kind, ptr(logits), ptr(lab) if kind != 2 else None, B, N, scale, shift, ptr(g),
             1 if g.dtype == torch.float64 else 0, ptr(d), stream())
        return d, None, None, None, None


_INFONCE_WS = {}


def infonce_uses_gemm(G: int, N: int) -> bool:
    """Large groups (in-batch contrast) go through the MFMA GEMMs; many small groups stay in the one-workgroup-per-group
    kernel whose logits live in LDS."""
    return N > infonce_max_n() or (N > 32 and G < 32)


def _infonce_ws(device, N, D):
    from ._lib import lib
    return _device_ws(_INFONCE_WS, device, lib().sbr_infonce_gemm_workspace(N, D), torch.uint8)


def infonce_fwd(a_ptr, b_ptr, ld, G, N, D, tau, scale, loss_out, device, gemm=None):
    """``gemm``: None chooses by ``infonce_uses_gemm``; False asks for the one-workgroup-per-group entry, which has a fixed-order form
    and takes N <= ``infonce_max_n()``"""
    if infonce_uses_gemm(G, N) if gemm is None else gemm:
        ws = _infonce_ws(device, N, D)
        call('sbr_infonce_gemm_fwd', a_ptr, b_ptr, ld, G, N, D, tau, scale, ptr(loss_out), ptr(ws), ws.numel(), stream())
    else:
        call('sbr_infonce_fwd', a_ptr, b_ptr, ld, G, N, D, tau, scale, ptr(loss_out), stream())


def infonce_bwd(a_ptr, b_ptr, ld, G, N, D, tau, scale, gout, da_ptr, db_ptr, ldg, device, gemm=None):
    if infonce_uses_gemm(G, N) if gemm is None else gemm:
        ws = _infonce_ws(device, N, D)
        call('sbr_infonce_gemm_bwd', a_ptr, b_ptr, ld, G, N, D, tau, scale, ptr(gout), da_ptr, db_ptr, ldg, ptr(ws), ws.numel(),
             stream())
    else:
        call('sbr_infonce_bwd', a_ptr, b_ptr, ld, G, N, D, tau, scale, ptr(gout), da_ptr, db_ptr, ldg, stream())


class InfoNCEFn(Function):
    """train/regularization_losses.py:14-43 on two [G, N, D] views that may be strided slices of one [G*N, 2, D] tensor. ``gemm``: the
    route, as in ``infonce_fwd`` (None: by ``infonce_uses_gemm``)."""

    @staticmethod
    def forward(ctx, e, tau: float, mean: bool, G: int, N: int, gemm=None):
        # e: [G*N, 2, D] contiguous; a = e[:, 0], b = e[:, 1]
        _need_cuda(e)
        e = _f32c(e)
        D = e.shape[-1]
        out = torch.empty((), device=e.device, dtype=torch.float64)
        scale = 1.0 / (G * N) if mean else 1.0
        infonce_fwd(e[:, 0].data_ptr(), e[:, 1].data_ptr(), 2 * D, G, N, D, tau, scale, out, e.device, gemm)
        ctx.args = (tau, scale, G, N, D, gemm)
        ctx.save_for_backward(e)
        return out.float()

    @staticmethod
    def backward(ctx, g):
        (e,) = ctx.saved_tensors
        tau, scale, G, N, D, gemm = ctx.args
        g = g.float().contiguous()
        de = torch.empty_like(e)
        infonce_bwd(e[:, 0].data_ptr(), e[:, 1].data_ptr(), 2 * D, G, N, D, tau, scale, g, de[:, 0].data_ptr(),
                    de[:, 1].data_ptr(), 2 * D, e.device, gemm)
        return de, None, None, None, None, None


def infonce_max_n() -> int:
    from ._lib import lib
    return lib().sbr_infonce_max_n()


# ---- evaluation helpers -----------------------------------------------------------------------------------------------------
def mask_scores_(scores: torch.Tensor, u_idx: torch.Tensor, excl_indptr: torch.Tensor, excl_indices: torch.Tensor, item_offset: int = None):
    """``item_offset`` (item-sharded evaluation): ``scores`` holds the item columns [item_offset, item_offset + scores.shape[1])."""
    _need_cuda(scores)
    if item_offset is None:
        call('sbr_mask_scores', ptr(scores), scores.stride(0), ptr(u_idx), ptr(excl_indptr), ptr(excl_indices), scores.shape[0], stream())
    else:
        call('sbr_mask_scores_shard', ptr(scores), scores.stride(0), ptr(u_idx), ptr(excl_indptr), ptr(excl_indices), scores.shape[0],
             int(item_offset), int(scores.shape[1]), stream())
    return scores


def topk_rows(scores: torch.Tensor, k: int):
    _need_cuda(scores)
    Bu, I = scores.shape
    val = torch.empty(Bu, k, device=scores.device, dtype=torch.float32)
    idx = torch.empty(Bu, k, device=scores.device, dtype=torch.int32)
    call('sbr_topk_rows', ptr(scores), scores.stride(0), Bu, I, k, ptr(val), ptr(idx), stream())
    return val, idx


def _need_vec(who, name, t, dtype, n=None):
    if not torch.is_tensor(t) or t.dtype != dtype or t.dim() != 1 or not t.is_contiguous() or (n is not None and t.numel() != n):
        got = f'{t.dtype} {tuple(t.shape)}' if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f'{who}: {name} must be a contiguous {dtype} vector' + (f' of {n} entries' if n is not None else '') + f', got {got}')


def shared_ranking(score: torch.Tensor) -> torch.Tensor:
    """-> int32 [n]: the stable descending order of a finite float32 vector under the rule of ``sbr_topk_rows`` — equal scores and the two
    zeros go in ascending index, which is what ``torch.sort(descending=True, stable=True)`` gives (include/sibrar_hip.h). The ranking
    ``shared_rank_topk`` walks; made once per catalogue, not per user. Non-finite input raises ``ValueError``."""
    _need_cuda(score)
    _need_vec('shared_ranking', 'score', score, torch.float32)
    if not bool(torch.isfinite(score).all()):
        raise ValueError('shared_ranking: non-finite scores')
    return torch.sort(score, descending=True, stable=True)[1].to(torch.int32)


def shared_rank_topk(order: torch.Tensor, score: torch.Tensor, u_idx: torch.Tensor, excl_indptr: torch.Tensor, excl_indices: torch.Tensor,
                     k: int):
    """-> (val float32 [Bu, k], idx int32 [Bu, k]): per user the first ``k`` entries of the shared ranking ``order`` (int32, positions,
    best first) that the user's exclusion row does not contain, with ``score`` (float32, by position) as their values; (-inf, -1) behind a
    user's last scoreable item (``sbr_shared_rank_topk``). The exclusion CSR is the one ``mask_scores_`` takes."""
    _need_cuda(order, score, u_idx, excl_indptr, excl_indices)
    who = 'shared_rank_topk'
    _need_vec(who, 'score', score, torch.float32)
    _need_vec(who, 'order', order, torch.int32, score.numel())
    _need_vec(who, 'u_idx', u_idx, torch.int64)
    _need_vec(who, 'excl_indptr', excl_indptr, torch.int64)
    _need_vec(who, 'excl_indices', excl_indices, torch.int32)
    if int(k) != k or k < 1:
        raise ValueError(f'{who}: k={k!r} must be an integer >= 1')
    Bu, k = u_idx.numel(), int(k)
    val = torch.empty(Bu, k, device=score.device, dtype=torch.float32)
    idx = torch.empty(Bu, k, device=score.device, dtype=torch.int32)
    call('sbr_shared_rank_topk', ptr(order), ptr(score), score.numel(), ptr(u_idx), ptr(excl_indptr), ptr(excl_indices), Bu, k, ptr(val),
         ptr(idx), stream())
    return val, idx


def uniform_rows(seed: int, u_idx: torch.Tensor, n_items: int) -> torch.Tensor:
    """-> float32 [Bu, n_items]: ``out[b, j] = U(seed, u_idx[b], j)`` in [0, 1), Philox4x32-10 keyed by ``seed`` with the counter
    (user id, j / 4) (``sbr_uniform_rows_f32``): a value depends on the seed, the user id and the item position only."""
    _need_cuda(u_idx)
    _need_vec('uniform_rows', 'u_idx', u_idx, torch.int64)
    if int(seed) != seed or not 0 <= seed < 1 << 64:
        raise ValueError(f'uniform_rows: seed={seed!r} must be an integer in [0, 2^64)')
    if int(n_items) != n_items or not 0 <= n_items < 1 << 31:
        raise ValueError(f'uniform_rows: n_items={n_items!r} must be an integer in [0, 2^31)')
    out = torch.empty(u_idx.numel(), int(n_items), device=u_idx.device, dtype=torch.float32)
    call('sbr_uniform_rows_f32', int(seed), ptr(u_idx), u_idx.numel(), int(n_items), ptr(out), out.stride(0) if out.numel() else int(n_items),
         stream())
    return out


def rank_metrics(topk_idx: torch.Tensor, u_idx, label_indptr, label_indices, ks: Sequence[int]):
    _need_cuda(topk_idx)
    Bu, kmax = topk_idx.shape
    import ctypes
    ks_arr = (ctypes.c_int * len(ks))(*ks)
    out = torch.empty(3, len(ks), Bu, device=topk_idx.device, dtype=torch.float32)
    call('sbr_rank_metrics', ptr(topk_idx), kmax, ptr(u_idx), ptr(label_indptr), ptr(label_indices), Bu,
         ctypes.cast(ks_arr, ctypes.c_void_p), len(ks), ptr(out), stream())
    return out


def rank_metrics_pos(topk_idx: torch.Tensor, u_idx, label_indptr, label_indices, ks: Sequence[int]):
    """-> float32 [3, n_ks, Bu]: dcg, ap and rr at every cut-off of ``ks`` (``sbr_rank_metrics_pos``; the operands of ``rank_metrics``)"""
    _need_cuda(topk_idx)
    Bu, kmax = topk_idx.shape
    import ctypes
    ks_arr = (ctypes.c_int * len(ks))(*ks)
    out = torch.empty(3, len(ks), Bu, device=topk_idx.device, dtype=torch.float32)
    call('sbr_rank_metrics_pos', ptr(topk_idx), kmax, ptr(u_idx), ptr(label_indptr), ptr(label_indices), Bu,
         ctypes.cast(ks_arr, ctypes.c_void_p), len(ks), ptr(out), stream())
    return out


def cast_f16(x: torch.Tensor) -> torch.Tensor:
    _need_cuda(x)
    x = _f32c(x)
    y = torch.empty(x.shape, device=x.device, dtype=torch.float16)
    call('sbr_cast_f32_to_f16', ptr(x), ptr(y), x.numel(), stream())
    return y


class ScorerExclusions:
    """The exclusion mask of one (user list, exclusion CSR, item range) combination in the layout the fused scorer reads (a
    wave-uniform event stream, csrc/score_topk_f16_n.hip). The mask of an evaluation split never changes (eval/eval.py:219:
    ``dataset.exclude_data``), so ``evaluation.evaluate_recommender_algorithm`` keeps one of these per (split, user chunk, item
    shard) next to the resident CSR and every evaluation after the first skips the three builder launches. The first
    ``score_topk_f16`` call that receives the object builds the stream; later calls must pass the same u_idx / CSR / item range / D."""

    def __init__(self):
        self.buf, self.key = None, None


def _scorer_events(exclusions, key, Bu, nnz, device):
    """-> (event buffer or None, build flag) for one fused-scorer call. ``key`` names the route and its geometry first: the two routes
    lay the stream out for different tile widths, so a holder built for one is rebuilt, never reused, by the other."""
    if nnz <= 0:
        return None, 1
    holder = exclusions if exclusions is not None else ScorerExclusions()
    if holder.buf is not None and holder.key == key:
        return holder.buf, 0                   # built by an earlier call for the same users / mask / item range (the caller's promise)
    holder.buf = torch.empty(int(lib().sbr_score_topk_f16_events_bytes(Bu, nnz)) + 16, device=device, dtype=torch.uint8)
    holder.key = key
    return holder.buf, 1


def score_topk_route(route: int = -1) -> int:
    """Which fused scorer ``score_topk_f16`` runs (process-wide; returns the previous setting): 0 automatic — the one-pass kernel for
    every shape until the two-pass scorer (csrc/score_topk_f16_2p.hip) is the faster one —, 1 always one-pass, 2 two-pass (catalogues
    of >= 8,192 items) or an error; -1 only queries. Both return the same lists bit for bit; the switch exists for tests and A/B timing."""
    return int(lib().sbr_score_topk_f16_route(int(route)))


def _score_topk_fused(entry: str, route: str, u: torch.Tensor, i_op: torch.Tensor, I: int, k: int, u_idx, excl_indptr, excl_indices,
                      item_offset: int, exclusions):
    """One call of a fused scorer C entry (``entry`` and ``entry + '_workspace'``): output, workspace and exclusion-event plumbing
    shared by ``score_topk_f16``, ``score_topk_f32s`` and ``score_topk_f32s_d256``. ``route`` keys the cached event stream (the routes lay it out for different
    tile widths)."""
    Bu, D = u.shape
    val = torch.empty(Bu, k, device=u.device, dtype=torch.float32)
    idx = torch.empty(Bu, k, device=u.device, dtype=torch.int32)
    nnz = 0 if excl_indices is None else int(excl_indices.numel())
    if nnz == 0:
        # an empty CSR masks nothing: pass none (its empty index tensor has a NULL data pointer, which the C entries refuse next to a
        # non-NULL indptr: "exclusion CSR must be given whole or not at all")
        excl_indptr = excl_indices = None
    ws = torch.empty(max(int(getattr(lib(), entry + '_workspace')(Bu, I, k)), 8), device=u.device, dtype=torch.uint8)
    ev, build = _scorer_events(exclusions, (route, Bu, I, D, int(item_offset), nnz), Bu, nnz, u.device)
    _timed((entry[len('sbr_'):], Bu, I, D, k),
           lambda: call(entry, ptr(u), ptr(i_op), D, Bu, I, ptr(u_idx), ptr(excl_indptr), ptr(excl_indices), nnz, item_offset, k,
                        ptr(val), ptr(idx), ptr(ws), ws.numel(), ptr(ev), 0 if ev is None else ev.numel(), build, stream()))
    return val, idx


def score_topk_f16(u16: torch.Tensor, i16: torch.Tensor, k: int, u_idx=None, excl_indptr=None, excl_indices=None,
                   item_offset: int = 0, exclusions: 'ScorerExclusions' = None):
    """The fused fp16 scorer: ``[Bu, k]`` (scores descending, ties by ascending item position; ``(-inf, -1)`` behind fewer than k
    scoreable items). D in {64, 128, 256}, k <= 128 (k > 32 runs the wide kernels; the opt-in two-pass route takes k <= 32)."""
    _need_cuda(u16, i16)
    return _score_topk_fused('sbr_score_topk_f16', 'f16', u16, i16, i16.shape[0], k, u_idx, excl_indptr, excl_indices, item_offset,
                             exclusions)


def split_bf16x3(x: torch.Tensor) -> torch.Tensor:
    """fp32 [..., D] -> bfloat16 [3, ..., D]: three planes (round to nearest even each) whose sum is x — exactly for x = 0 and
    2^-100 <= |x| <= 3.38e38 (the item operand of ``score_topk_f32s``). Below 2^-100 the third plane underflows bf16 and the sum is
    x only to ~2^-133 absolute; above ~3.3961e38 the first plane rounds to inf and the sum is NaN; inf and NaN give (x, NaN, NaN).
    tests/test_hip_rowops.py asserts the range. Non-finite values are therefore NOT supported by the fp32-class scorer (every score
    of such an item row is NaN): check with ``split_bf16x3_supported`` and use the 'fp32' route instead, as the evaluator does."""
    _need_cuda(x)
    x = _f32c(x)
    y = torch.empty((3,) + tuple(x.shape), device=x.device, dtype=torch.bfloat16)
    call('sbr_split_f32_to_bf16x3', ptr(x), ptr(y), x.numel(), stream())
    return y


def split_bf16x3_supported(x: torch.Tensor) -> bool:
    """True when every value of x is finite and within the first plane's range (|x| <= 3.38e38): the bf16 split of anything else
    holds NaN planes (one reduction and one host read; the evaluator asks once per evaluation, where the planes are built)."""
    return bool((x.abs() <= 3.38e38).all())


def score_topk_f32s_supported(D: int, k: int) -> bool:
    return D in (64, 128) and 1 <= k <= 32


FUSED_MAX_K = 128                 # longest list the one-pass fused scorers build (the wide instantiations: 33 .. 128)
_FUSED_DIMS = {'fp16_fused': (64, 128, 256), 'fp32_fused': (64, 128)}


def check_fused_max_k(max_k) -> int:
    """``fused_max_k`` of the evaluator / trainer: an integer in [32, 128], anything else raises ValueError."""
    if isinstance(max_k, bool) or not isinstance(max_k, numbers.Integral) or not 32 <= int(max_k) <= FUSED_MAX_K:
        raise ValueError(f'fused_max_k must be an integer in [32, {FUSED_MAX_K}], got {max_k!r}')
    return int(max_k)


FUSED_MAX_D = 256                 # widest representation of the fp32-class fused route (score_topk_f32s_d256, on request)


def check_fused_max_d(max_d) -> int:
    """``fused_max_d`` of the evaluator / trainer: 128 or 256, anything else raises ValueError."""
    if isinstance(max_d, bool) or not isinstance(max_d, numbers.Integral) or int(max_d) not in (128, FUSED_MAX_D):
        raise ValueError(f'fused_max_d must be 128 or {FUSED_MAX_D}, got {max_d!r}')
    return int(max_d)


def score_topk_fused_supported(route: str, D: int, k: int, max_k: int = 32, max_d: int = 128) -> bool:
    """Whether the fused scorer ``route`` ('fp16_fused' / 'fp32_fused') takes representations of width D and lists of k entries when the
    caller allows lists up to ``max_k`` (32: the evaluator's default, longer lists go to the fp32 route; up to 128: the wide kernels)
    and, on 'fp32_fused', representations up to ``max_d`` wide (128: the default, D = 256 goes to the fp32 route; 256: the
    one-wave-per-SIMD kernels of ``score_topk_f32s_d256``)."""
    if route not in _FUSED_DIMS:
        raise ValueError(f'unknown fused scorer {route!r}')
    dims = _FUSED_DIMS[route]
    if check_fused_max_d(max_d) == FUSED_MAX_D and route == 'fp32_fused':
        dims = dims + (FUSED_MAX_D,)
    return int(D) in dims and 1 <= int(k) <= check_fused_max_k(max_k)


def score_topk_f32s(u32: torch.Tensor, i_planes: torch.Tensor, k: int, u_idx=None, excl_indptr=None, excl_indices=None,
                    item_offset: int = 0, exclusions: 'ScorerExclusions' = None):
    """The fused scorer with fp32-class products (eval/eval.py:216-222): fp32 user rows ``u32`` [Bu, D] against the item planes
    ``i_planes`` = ``split_bf16x3(items)`` [3, I, D]; the output contract of ``score_topk_f16``. D in {64, 128}, k <= 128."""
    _need_cuda(u32, i_planes)
    u32 = _f32c(u32)
    Bu, D = u32.shape
    if i_planes.dtype != torch.bfloat16 or i_planes.dim() != 3 or i_planes.shape[0] != 3 or i_planes.shape[2] != D:
        raise ValueError(f'score_topk_f32s: item planes must be bfloat16 [3, I, {D}] (split_bf16x3), got {i_planes.dtype} {tuple(i_planes.shape)}')
    i_planes = i_planes.contiguous()
    return _score_topk_fused('sbr_score_topk_f32s', 'f32s', u32, i_planes, i_planes.shape[1], k, u_idx, excl_indptr, excl_indices,
                             item_offset, exclusions)


def score_topk_f32s_d256(u32: torch.Tensor, i_planes: torch.Tensor, k: int, u_idx=None, excl_indptr=None, excl_indices=None,
                         item_offset: int = 0, exclusions: 'ScorerExclusions' = None):
    """``score_topk_f32s`` for 256-wide representations (eval/eval.py:216-222): the same arithmetic and output contract from kernels
    of their own (one wave per SIMD: the user planes take 192 registers). D = 256 only, k <= 128."""
    _need_cuda(u32, i_planes)
    u32 = _f32c(u32)
    Bu, D = u32.shape
    if D != 256:
        raise ValueError(f'score_topk_f32s_d256: D={D} not supported (256; score_topk_f32s has 64 and 128)')
    if i_planes.dtype != torch.bfloat16 or i_planes.dim() != 3 or i_planes.shape[0] != 3 or i_planes.shape[2] != D:
        raise ValueError(f'score_topk_f32s_d256: item planes must be bfloat16 [3, I, {D}] (split_bf16x3), got {i_planes.dtype} {tuple(i_planes.shape)}')
    i_planes = i_planes.contiguous()
    return _score_topk_fused('sbr_score_topk_f32s_d256', 'f32s_d256', u32, i_planes, i_planes.shape[1], k, u_idx, excl_indptr, excl_indices,
                             item_offset, exclusions)


# ---- optimizer steps ----------------------------------------------------------------------------------------------------------
def adam_step(kind: int, p, g, m, v, lr, b1, b2, eps, wd, step: int, zero_grad: bool = False, copy=None):
    """One dense Adam / AdamW step; ``zero_grad``: the gradient is reset by the same launch (step() + zero_grad());
    ``copy`` = (src, dst) float64 tensors of <= 256 elements (needs ``zero_grad``): copied by the same launch."""
    if zero_grad:
        src, dst = copy if copy is not None else (None, None)
        call('sbr_adam_step_zero_grad', kind, ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, b1, b2, eps, wd, step, ptr(src), ptr(dst),
             0 if src is None else src.numel(), stream())
    else:
        assert copy is None
        call('sbr_adam_step', kind, ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, b1, b2, eps, wd, step, stream())


def adagrad_step(p, g, s, lr, eps, wd):
    call('sbr_adagrad_step', ptr(p), ptr(g), ptr(s), p.numel(), lr, eps, wd, stream())
