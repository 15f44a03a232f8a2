"""GPU: the high-water rule of sbr_raise_lds (csrc/common.h) on the two InfoNCE kernels whose dynamic LDS size depends on run-time
arguments (csrc/loss.hip). A kernel's limit is raised only on another device or for MORE bytes than it was last raised to, so a
sequence of calls that goes below 64 KiB, above it, to the maximum and then lower again must launch every time — in this fixed order,
inside one test function, because the slot is a process-wide static.

Both functions call the C entries sbr_infonce_fwd / sbr_infonce_bwd directly, as tests/test_hip_tail.py does: ops.infonce_fwd sends
few large groups (N > 32 with G < 32) to the GEMM route, which has no LDS-resident logits. Inside the entry, N > 16 fails
infonce_small_ok, so infonce_kernel runs; N <= 16 with D <= 256, D % 4 == 0 and 16-byte aligned rows passes it, so infonce_small_kernel
runs. Results are held to the float64 reference and bounds of test_infonce_lds_routes_against_float64 (tests/test_hip_tail.py).

infonce_small_lds(N, D) = 16 (2 N (D + 4) + N (N + 1) + 2 N + 2) bytes admits pairs on both sides of 64 KiB: N = 16 with D = 64
(39,712 bytes) and D = 128 (72,480) or D = 256 (138,016)."""
import numpy as np
import pytest
import torch

from hip_testutil import DEV, NAN, U32, S, _L, _assert_bound, _Buf, _p, _rand, call, stream
from test_hip_tail import infonce_bounds, ref_infonce

pytestmark = pytest.mark.gpu


def _check(G, N, D, tau):
    """one forward and one backward at (G, N, D) against float64; -> nothing"""
    a, b = _rand(G, N, D, seed=N + D) * 0.5, _rand(G, N, D, seed=N + D + 1) * 0.5
    scale = 1.0 / (G * N)
    A, B = _Buf(G * N, D, data=a.reshape(G * N, D)), _Buf(G * N, D, data=b.reshape(G * N, D))
    dA, dB = _Buf(G * N, D), _Buf(G * N, D)
    tau32 = float(np.float32(tau))
    loss_ref, da_ref, db_ref, _, _ = ref_infonce(a.double(), b.double(), tau32, scale)
    bl, bA, bB = infonce_bounds(a.double(), b.double(), tau32, scale)
    lo = torch.full((1,), 5.0, dtype=torch.float64, device=DEV)
    gout = torch.ones(1, device=DEV)
    what = f'N {N} D {D}'
    call('sbr_infonce_fwd', A.ptr, B.ptr, D, G, N, D, tau, scale, _p(lo), stream())
    print(what, 'loss err', abs(float(lo) - float(loss_ref)), 'bound', float(bl))
    assert abs(float(lo) - float(loss_ref)) <= float(bl), (what, float(lo), float(loss_ref), float(bl))
    dA.flat.fill_(NAN)
    dB.flat.fill_(NAN)
    call('sbr_infonce_bwd', A.ptr, B.ptr, D, G, N, D, tau, scale, _p(gout), dA.ptr, dB.ptr, D, stream())
    ga, gb = dA.check_untouched(None, 'dA'), dB.check_untouched(None, 'dB')
    _assert_bound(ga.reshape(G, N, D), da_ref, bA + 3 * U32 * da_ref.abs(), 'dA ' + what)
    _assert_bound(gb.reshape(G, N, D), db_ref, bB + 3 * U32 * db_ref.abs(), 'dB ' + what)


def _entries(log):
    return [name for name, _ in log]


def test_infonce_kernel_lds_limit_high_water():
    """infonce_kernel, infonce_lds(N) = 4 (N (N + 1) + 2 N): N = 126 (65,016 bytes, under the 64 KiB every kernel has), 128 (67,072: the
    first raise), 176 (126,016: the maximum), 130 (69,160: lower again, no new raise) — every launch runs and is right."""
    L = _L()
    assert S().ops.infonce_max_n() == 176
    G, D = 2, 8
    prev, L.CALL_LOG = L.CALL_LOG, []
    try:
        for N in (126, 128, 176, 130):
            assert N > 16 and 4 * (N * (N + 1) + 2 * N) == {126: 65016, 128: 67072, 176: 126016, 130: 69160}[N]
            _check(G, N, D, 0.3)
        assert _entries(L.CALL_LOG) == ['sbr_infonce_fwd', 'sbr_infonce_bwd'] * 4
    finally:
        L.CALL_LOG = prev


def test_infonce_small_kernel_lds_limit_high_water():
    """infonce_small_kernel (N <= 16, D <= 256, D % 4 == 0, aligned rows): D = 64 (39,712 bytes), 128 (72,480: the first raise), 256
    (138,016), 128 again (lower, no new raise)."""
    L = _L()
    G, N = 5, 16
    prev, L.CALL_LOG = L.CALL_LOG, []
    try:
        for D in (64, 128, 256, 128):
            assert not S().ops.infonce_uses_gemm(G, N) and N <= 16 and D <= 256 and D % 4 == 0
            assert 16 * (2 * N * (D + 4) + N * (N + 1) + 2 * N + 2) == {64: 39712, 128: 72480, 256: 138016}[D]
            _check(G, N, D, 0.3)
        assert _entries(L.CALL_LOG) == ['sbr_infonce_fwd', 'sbr_infonce_bwd'] * 4
    finally:
        L.CALL_LOG = prev
