"""In-process A/B of the bf16-split GEMM family (csrc/gemm_split_*.hip) at the shapes of the training step, between the product library
and every tools/lab/bin/libsibrar_*.so. The use case is a library built from ANOTHER COMMIT and copied there (two copies of it give the
noise of the box: their difference is the margin for any verdict). Every entry point runs on seeded six-decade operands; the libraries
are timed in rotation with HIP events. Per entry and library: the median over the rounds, every round's median, and whether the output
bits equal the product's (the pending double column sums are arrival-order atomics: their error against the bound of
tests/test_hip_gemm.py::test_wres_split_y_epilogue_and_colsum is printed instead).
usage: python tools/lab/gemm_split_ab.py [rounds]"""
import ctypes, glob, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
import sibrar_amd as S
from importlib import import_module
L = import_module('sibrar---single-branch-recommender_amd._lib')
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
REPS = 10
dev = 'cuda:0'
g = torch.Generator().manual_seed(3)
hdr = L.parse_header()
paths = {'product': L.LIB_PATH}
for p in sorted(glob.glob(os.path.join(ROOT, 'tools', 'lab', 'bin', 'libsibrar_*.so'))):
    paths[os.path.basename(p)[len('libsibrar_'):-3]] = p
libs = {name: ctypes.CDLL(p) for name, p in paths.items()}
stream = torch.cuda.current_stream().cuda_stream


def fn(lib, name):
    f = getattr(libs[lib], name)
    f.restype, f.argtypes = hdr[name][0], hdr[name][1]
    return f


def six(*shape):                                    # magnitudes over six decades
    return (torch.randn(*shape, generator=g) * 10.0 ** (torch.rand(*shape, generator=g) * 6 - 3)).to(dev)


def p(t):
    return None if t is None else t.data_ptr()


R, RP, ROWS = 90112, 45824, 50_000
A128, Y128 = six(R, 128), torch.relu(six(R, 128))
W128, b128 = six(128, 128), six(128)
X768, W768 = six(ROWS, 768), six(128, 768)
a_idx = torch.randint(0, ROWS, (RP,), generator=g, dtype=torch.int32).to(dev)
c_idx = torch.randperm(2 * RP, generator=g)[:RP].to(torch.int32).to(dev)
A512, W512, b512 = six(R, 512), six(512, 512), six(512)


def gemm128(mode, with_y):
    def make(lib):
        C = torch.zeros(R, 128, device=dev)
        ws = torch.zeros(17 * 128, device=dev, dtype=torch.float64) if with_y else None
        f = fn(lib, 'sbr_gemm_split_f32')

        def run():
            if ws is not None:
                ws.zero_()
            rc = f(mode, p(A128), 128, p(W128), 128, p(b128) if mode == 0 else None, p(C), 128, R, 128, 128, 1, p(Y128) if with_y else None,
                   128 if with_y else 0, p(ws), stream)
            assert rc == 0, rc
        return run, {'C': C}, ({'colsum': (ws, C)} if with_y else {})
    return make


def bnstats(lib):
    C = torch.zeros(R, 128, device=dev)
    ws = torch.zeros(17 * 2 * 128, device=dev, dtype=torch.float64)
    arrive = torch.zeros(1, device=dev, dtype=torch.int64)
    mean, rstd = torch.zeros(128, device=dev), torch.zeros(128, device=dev)
    f = fn(lib, 'sbr_gemm_split_bnstats_f32')

    def run():
        rc = f(p(A128), 128, p(W128), 128, p(b128), p(C), 128, R, 128, 128, 1, p(ws), p(arrive), None, None, None, p(mean), p(rstd), 1e-5, 0.1, stream)
        assert rc == 0, rc
    return run, {'C': C, 'save_mean': mean, 'save_rstd': rstd, 'replicas left': ws, 'arrive left': arrive}, {}


def proj(gather, scatter):
    def make(lib):
        C = torch.zeros(2 * RP, 128, device=dev)
        f = fn(lib, 'sbr_gemm_split_proj_f32')

        def run():
            rc = f(p(X768), 768, p(a_idx) if gather else None, p(W768), 768, p(b128), p(C), 128, p(c_idx) if scatter else None, RP, 128, 768, 1, stream)
            assert rc == 0, rc
        return run, {'C': C}, {}
    return make


def tn(A, B, b_rows, N, K):
    def make(lib):
        nbytes = fn(lib, 'sbr_gemm_tn_f32_workspace')(128, N, K)
        ws = torch.zeros(nbytes // 4, device=dev)
        splits = ctypes.c_int(0)
        f = fn(lib, 'sbr_gemm_tn_f32_slabs')

        def run():
            rc = f(p(A), 128, None, p(B), N, p(b_rows), 128, N, K, p(ws), nbytes, ctypes.byref(splits), stream)
            assert rc == 0, rc
        return run, {'slabs': ws}, {}
    return make


def wide(mode):
    def make(lib):
        C = torch.zeros(R, 512, device=dev)
        f = fn(lib, 'sbr_gemm_split_wide_f32')

        def run():
            rc = f(mode, p(A512), 512, None, p(W512), 512, p(b512) if mode == 0 else None, p(C), 512, None, R, 512, 512, 1 if mode == 0 else 0, stream)
            assert rc == 0, rc
        return run, {'C': C}, {}
    return make


CASES = [('split NT 90112x128x128', gemm128(0, False)), ('split NN', gemm128(1, False)), ('split NN + Y', gemm128(1, True)),
         ('bnstats 90112x128x128', bnstats), ('proj 45824x128x768 gathered', proj(True, False)), ('proj scattered', proj(False, True)),
         ('tn 128x128 over 90112', tn(A128, Y128, None, 128, R)), ('tn 128x768 over 45824 gathered', tn(A128, X768, a_idx, 768, RP)),
         ('wide NT 90112x512x512', wide(0)), ('wide NN', wide(1))]
only = os.environ.get('AB_ONLY', '')
for title, make in CASES:
    if only not in title:
        continue
    made = {lib: make(lib) for lib in libs}
    for lib in libs:
        made[lib][0]()
    torch.cuda.synchronize()
    notes = {}
    for lib in libs:
        same = [k for k, t in made[lib][1].items() if torch.equal(t.view(torch.int32) if t.dtype == torch.float32 else t,
                                                                  made['product'][1][k].view(torch.int32) if t.dtype == torch.float32 else made['product'][1][k])]
        diff = [k for k in made[lib][1] if k not in same]
        notes[lib] = 'bits equal' if not diff else 'BITS DIFFER: ' + ', '.join(diff)
        for k, (ws, C) in made[lib][2].items():
            got, ref = ws.view(17, 128)[1:].sum(0), C.double().sum(0)
            bound = (16 * 2.0 ** -24 / (1 - 16 * 2.0 ** -24) + 1e-12) * C.double().abs().sum(0)
            notes[lib] += f'; {k} error / bound {((got - ref).abs() / bound).max().item():.3f}'
    times = {lib: [] for lib in libs}
    for r in range(ROUNDS):
        for lib in libs:
            run = made[lib][0]
            for _ in range(3):
                run()
            evs = []
            for _ in range(REPS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); run(); e1.record()
                evs.append((e0, e1))
            torch.cuda.synchronize()
            ts = sorted(a.elapsed_time(b) * 1e3 for a, b in evs)
            times[lib].append(ts[len(ts) // 2])
    print(title)
    for lib, ts in times.items():
        print(f'  {lib:10s} median {sorted(ts)[len(ts) // 2]:7.1f} us  rounds {" ".join(f"{x:.1f}" for x in ts)}  {notes[lib]}', flush=True)
    del made
    torch.cuda.empty_cache()
