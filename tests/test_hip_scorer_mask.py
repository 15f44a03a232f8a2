"""GPU: the exclusion mask of the fused scorers (sbr_score_topk_f16 one-pass and two-pass, sbr_score_topk_f32s, sbr_score_topk_f32s_d256)
and the reuse of its event stream, bit for bit against an integer oracle.

All four kernels apply the mask through the event stream of csrc/score_topk_shared.h (s5_ev_rows_kernel, s5_ev_scan_kernel,
s5_ev_scatter_kernel), read by StEvents (csrc/score_topk_stream.h) and by pass 1 of csrc/score_topk_f16_2p.hip. The operands are the
integer-score construction of tests/scorer_mask_cases.py (pinned on the CPU by tests/test_scorer_mask_cpu.py): every route returns the
same exactly representable scores, so every list equals ``expected_lists`` in bits, and over the rounds of the rotation every
(user, item) mask bit is observed — an item of the unexcluded top-k window that is missing from a user's list was masked, one that is
listed was not. Outputs, workspace and event buffer of every C call are views into pattern-filled allocations.

Edges and the case that covers them:
  group event counts 0, 1, 3, 4, 5, 7, 8, 9, an empty middle group, ragged last groups ........ quad-Bu{96, 1, 31, 32, 33, 65}
  a tile with every score excluded, a user with the whole shard excluded ...................... fulltile
  columns 0, T - 1, T, 2 T - 1, I - 1 and the partial last tile ............................... edges-T{64, 32}-I*
  the two binary searches that clip a CSR row to the shard (nine row kinds) ................... clip
  the u_idx map, with repeated rows ........................................................... uidx-distinct, uidx-repeat
  the prefix pass and its restart() ........................................................... test_prefix_pass_*
  the partial-wave plan: a part passes over other parts' events ............................... test_partial_wave_*
  the second consumer (two-pass fp16) ......................................................... test_two_pass_*
  build_events = 0 (C interface, ops.ScorerExclusions, the evaluator's per-split cache) ....... test_reuse_*"""
from contextlib import contextmanager
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import scorer_mask_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PAD = 4096
# route -> (C entry, D, tile width of the event stream, prefix-pass tiles)
ROUTES = {
    'f16-64': ('sbr_score_topk_f16', 64, 64, 16),
    'f16-128': ('sbr_score_topk_f16', 128, 64, 16),
    'f16-256': ('sbr_score_topk_f16', 256, 32, 16),
    'f32s-64': ('sbr_score_topk_f32s', 64, 32, 32),
    'f32s-128': ('sbr_score_topk_f32s', 128, 32, 32),
    'f32s_d256': ('sbr_score_topk_f32s_d256', 256, 32, 32),
}


def S():
    import sibrar_amd
    return sibrar_amd


def _L():
    return import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')


@contextmanager
def f16_route(route):
    prev = S().ops.score_topk_route(route)
    try:
        yield
    finally:
        S().ops.score_topk_route(prev)


class _Guarded:
    """``nbytes`` bytes inside an allocation of 0xFF bytes (as fp32: NaN, as int32: -1)"""

    def __init__(self, nbytes, what):
        n = max(int(nbytes), 16)
        self.what = what
        self.whole = torch.full((PAD + n + PAD,), 0xFF, dtype=torch.uint8, device=DEV)
        self.view = self.whole[PAD:PAD + n]

    def check(self):
        n = self.view.numel()
        assert bool((self.whole[:PAD] == 0xFF).all()) and bool((self.whole[PAD + n:] == 0xFF).all()), f'wrote outside its {self.what}'


def _csr_dev(m):
    return (torch.from_numpy(m.indptr.astype(np.int64)).to(DEV), torch.from_numpy(m.indices.astype(np.int32)).to(DEV))


def _operands(route, Bu, I):
    """-> (user operand, item rows BY RANK in the route's operand format): a round's item operand is a row gather of the table"""
    D = ROUTES[route][1]
    u, by_rank = C.operands(I, D, np.arange(I), Bu)
    u, by_rank = torch.from_numpy(u).to(DEV), torch.from_numpy(by_rank).to(DEV)
    if route.startswith('f16'):
        return u.half(), by_rank.half()
    return u, S().ops.split_bf16x3(by_rank)


def _items(route, table, rk):
    rk = torch.from_numpy(np.asarray(rk)).to(DEV)
    return table[rk].contiguous() if route.startswith('f16') else table[:, rk].contiguous()


_ORACLE = {}


def _oracle(c, k, a, r):
    """expected lists of one round of a case: computed once, shared by the routes that run the same case"""
    key = (c.name, c.Bu, c.I, c.item_offset, k, a, r)
    if key not in _ORACLE:
        _ORACLE[key] = C.expected_lists(C.scores(c.I, C.ranks(c.I, k, r, a)), C.dense_mask(c), k, c.item_offset)
    return _ORACLE[key]


class Run:
    """One (case, route): operands and guarded buffers made once, ``call`` = one launch of the C entry for one round's ranks."""

    def __init__(self, case, route):
        self.c, self.route = case, route
        self.entry, self.D, self.T, self.pre = ROUTES[route]
        self.ex = _csr_dev(case.csr)
        self.nnz = int(self.ex[1].numel())
        self.users = torch.from_numpy(case.u_idx).to(DEV)
        self.u, self.table = _operands(route, case.Bu, case.I)
        self.mask = C.dense_mask(case)
        lib = _L().lib()
        self.ev = _Guarded(int(lib.sbr_score_topk_f16_events_bytes(case.Bu, self.nnz)) + 16, 'event buffer')
        self.out = {}

    def _buffers(self, k):
        key = (k, S().ops.score_topk_route(-1))
        if key not in self.out:
            Bu = self.c.Bu
            ws = _Guarded(int(getattr(_L().lib(), self.entry + '_workspace')(Bu, self.c.I, k)), 'workspace')
            self.out[key] = (_Guarded(Bu * k * 4, 'value rows'), _Guarded(Bu * k * 4, 'index rows'), ws)
        return self.out[key]

    def call(self, k, rk, build):
        """-> (val, idx) device clones; asynchronous"""
        _lib = _L()
        gv, gi, ws = self._buffers(k)
        Bu = self.c.Bu
        val, idx = gv.view[:Bu * k * 4].view(torch.float32).view(Bu, k), gi.view[:Bu * k * 4].view(torch.int32).view(Bu, k)
        it = _items(self.route, self.table, rk)
        _lib.call(self.entry, _lib.ptr(self.u), _lib.ptr(it), self.D, Bu, self.c.I, _lib.ptr(self.users), _lib.ptr(self.ex[0]),
                  _lib.ptr(self.ex[1]), self.nnz, self.c.item_offset, k, _lib.ptr(val), _lib.ptr(idx), _lib.ptr(ws.view), ws.view.numel(),
                  _lib.ptr(self.ev.view), self.ev.view.numel(), int(build), _lib.stream())
        return val.clone(), idx.clone()

    def check_guards(self):
        torch.cuda.synchronize()
        self.ev.check()
        for bufs in self.out.values():
            for b in bufs:
                b.check()

    def rounds(self, k, plan, first_build=True):
        """``plan``: [(a, r)] in launch order. Every round's lists equal the oracle; -> the observed mask bits [Bu, I] and how often every
        item was observed. The stream is built by the first launch and reused (build_events = 0) by the others: it depends on the mask only."""
        c = self.c
        outs = [self.call(k, C.ranks(c.I, k, r, a), first_build and n == 0) for n, (a, r) in enumerate(plan)]
        vals = torch.stack([o[0] for o in outs]).cpu().numpy()       # one transfer for all rounds (synchronises)
        idxs = torch.stack([o[1] for o in outs]).cpu().numpy()
        seen = np.zeros(c.I, dtype=np.int64)
        obs = np.zeros((c.Bu, c.I), dtype=bool)
        for (a, r), val, idx in zip(plan, vals, idxs):
            want_v, want_i = _oracle(c, k, a, r)
            what = f'{c.name} {self.route} k={k} a={a} r={r}'
            bad = (idx != want_i).any(1) | (val.view(np.int32) != want_v.view(np.int32)).any(1)
            assert not bad.any(), (f'{what}: {int(bad.sum())} of {c.Bu} lists differ, first user {int(np.flatnonzero(bad)[0])}: got '
                                   f'{idx[bad][0].tolist()} {val[bad][0].tolist()}, expected {want_i[bad][0].tolist()} {want_v[bad][0].tolist()}')
            win = C.window(c.I, k, r, a)
            obs[:, win] = C.observed_mask(idx, win, c.item_offset)
            seen[win] += 1
        return obs, seen

    def rotation(self, k):
        """the full rotation for both stride families: every (user, item) mask bit observed, equal to the dense CSR mask"""
        c = self.c
        for a in (1, C.stride(c.I)):
            obs, seen = self.rounds(k, [(a, r) for r in range(C.n_rounds(c.I, k))])
            assert (seen == 1).all()
            bad = obs != self.mask
            assert not bad.any(), f'{c.name} {self.route} k={k} a={a}: observed mask differs at (user, item) {np.argwhere(bad)[:8].tolist()}'


def _patterns(T):
    cases = [C.quad_edges(Bu) for Bu in sorted(C.QUAD_COUNTS)]
    cases += [C.full_tile(T)]
    cases += [C.tile_edges(T, I) for I in C.TILE_EDGE_I[T]]
    cases += [C.shard_clip(), C.u_idx_map(False), C.u_idx_map(True)]
    return cases


_N_PATTERNS = len(_patterns(64))


@pytest.mark.parametrize('n', range(_N_PATTERNS))
@pytest.mark.parametrize('route', sorted(ROUTES))
def test_every_mask_bit_of_every_pattern_on_every_route(route, n):
    """k = 1, 10, 32 through the whole rotation: lists exact in every round, observed mask == dense CSR mask clipped to the shard."""
    case = _patterns(ROUTES[route][2])[n]
    with f16_route(1):
        run = Run(case, route)
        for k in (1, 10, 32):
            run.rotation(k)
        run.check_guards()


@pytest.mark.parametrize('route', sorted(ROUTES))
def test_wide_lists_through_the_rotation_and_by_direct_enumeration(route):
    """The wide instantiations: k = 33 on the quad-edge pattern of 96 users and k = 128 on the shard-clipping pattern through the
    rotation; on the tile-edge patterns with I <= k one launch lists every non-excluded item."""
    T = ROUTES[route][2]
    with f16_route(1):
        for k, case in ((33, C.quad_edges(96)), (128, C.shard_clip())):
            run = Run(case, route)
            run.rotation(k)
            run.check_guards()
        n_direct = 0
        for k in (33, 128):
            for I in C.TILE_EDGE_I[T]:
                if I > k:
                    continue
                run = Run(C.tile_edges(T, I), route)
                for a in (1, C.stride(I)):
                    obs, seen = run.rounds(k, [(a, 0)])
                    assert (seen == 1).all() and np.array_equal(obs, run.mask)
                run.check_guards()
                n_direct += 1
        assert n_direct >= 5


def _prefix_cases():
    return [(route, I) for route in sorted(ROUTES) for I in C.PREFIX_I[(ROUTES[route][2], ROUTES[route][3])]]


@pytest.mark.parametrize('route,I', _prefix_cases())
def test_prefix_pass_does_not_count_excluded_scores(route, I):
    """Catalogues just below, at and above the smallest one that runs the prefix pass (6 x PRE_TILES tiles), k = 20, 40 users that each
    exclude another subset of the 40 best scores of the round (a = 1, r = 0), which lie in the prefix tiles: an excluded score counted
    into a class maximum would raise the threshold and shorten or alter the list. The prefix pass reads the first tiles' events and
    restarts the cursor. One contiguous and one strided round."""
    _, _, T, pre = ROUTES[route]
    with f16_route(1):
        run = Run(C.prefix(I, T, pre), route)
        run.rounds(20, [(1, 0), (C.stride(I), 7), (1, 0)])
        run.check_guards()


@pytest.mark.parametrize('route', ['f16-64', 'f32s-64'])
def test_partial_wave_plan_passes_over_other_parts_events(route):
    """Bu = 32 (G + 1) on G compute units: one full wave per workgroup and ONE remainder unit cut into 8 parts by item tile (s5_plan);
    every user of that unit has an exclusion in every tile, so every part has to pass over the other parts' events. I = 300, k = 10."""
    G = int(torch.cuda.get_device_properties(0).multi_processor_count)
    assert G >= 16
    with f16_route(1):
        run = Run(C.partial_wave(G, ROUTES[route][2]), route)
        obs, seen = run.rounds(10, [(1, 0), (C.stride(300), 4)])
        run.check_guards()
    win = np.flatnonzero(seen)
    assert len(win) >= 10 and np.array_equal(obs[:, win], run.mask[:, win])


@pytest.mark.parametrize('D', [64, 128, 256])
def test_two_pass_route_reads_the_same_stream(D):
    """I = 8192 (the two-pass route's smallest catalogue), k = 10: quad-edge and shard-clipping patterns with exclusions in the first, a
    middle and the last tile; route 2 == route 1 bit for bit == the oracle."""
    route = f'f16-{D}'
    T = ROUTES[route][2]
    I = 8192
    cases = [C.quad_edges(Bu, I=I, cols=C.three_tile_cols(I, T)) for Bu in (96, 33, 65)] + [C.shard_clip(off=300, I=I)]
    plan = [(1, 0), (C.stride(I), 5)]
    for case in cases:
        got = {}
        for r in (1, 2):
            with f16_route(r):
                run = Run(case, route)
                run.rounds(10, plan)                                 # == the oracle
                got[r] = [run.call(10, C.ranks(I, 10, rr, a), False) for (a, rr) in plan]
                run.check_guards()
        for (v1, i1), (v2, i2) in zip(got[1], got[2]):
            assert torch.equal(i1, i2) and torch.equal(v1.view(torch.int32), v2.view(torch.int32)), f'{case.name}: two-pass differs from one-pass'


@pytest.mark.parametrize('route,fp16_route', [(r, 1) for r in sorted(ROUTES)] + [(r, 2) for r in sorted(ROUTES) if r.startswith('f16')])
def test_reuse_through_the_c_interface(route, fp16_route):
    """build_events = 1 into a guarded buffer, then two calls with build_events = 0, the same buffer and OTHER item ranks: every call
    equals its own oracle, the buffer's bytes are unchanged and the guards intact — the stream depends on the mask only."""
    I = 8192 if fp16_route == 2 else 200
    case = C.shard_clip(off=300, I=I)
    with f16_route(fp16_route):
        run = Run(case, route)
        run.rounds(10, [(1, 0)])
        built = run.ev.view.clone()
        assert bool((built != 0xFF).any())
        # the head of the buffer (csrc/score_topk_shared.h: group_base int[G + 1], grp_cnt int[G], 16-byte aligned pieces): every group
        # counts exactly the in-shard entries of its rows — one entry too many at either end of the shard shows here even where it lands
        # on a column no score has — and gets room for its events rounded up to a quad plus two padding quads
        G = -(-case.Bu // 32)
        head = built.cpu().numpy()
        a16 = (4 * (G + 1) + 15) & ~15
        cnt = C.group_counts(case)
        room = ((cnt + 3) & ~3) + 8
        assert head[a16:a16 + 4 * G].view(np.int32).tolist() == cnt.tolist(), 'group event counts'
        assert head[:4 * (G + 1)].view(np.int32).tolist() == [0] + np.cumsum(room).tolist(), 'group bases'
        run.rounds(10, [(1, 5), (C.stride(I), 11)], first_build=False)
        run.check_guards()
        assert torch.equal(run.ev.view, built), 'a build_events = 0 call wrote the event buffer'


def _ops_call(route, run, k, rk, holder, case=None):
    ops = S().ops
    c = case or run.c
    fn = {'sbr_score_topk_f16': ops.score_topk_f16, 'sbr_score_topk_f32s': ops.score_topk_f32s,
          'sbr_score_topk_f32s_d256': ops.score_topk_f32s_d256}[ROUTES[route][0]]
    it = _items(route, run.table, rk)
    users = torch.from_numpy(c.u_idx).to(DEV)
    val, idx = fn(run.u[:c.Bu], it, k, users, run.ex[0], run.ex[1], item_offset=c.item_offset, exclusions=holder)
    torch.cuda.synchronize()
    return val.cpu().numpy(), idx.cpu().numpy()


def _assert_exact(got, case, k, rk, what):
    want_v, want_i = C.expected_lists(C.scores(case.I, rk), C.dense_mask(case), k, case.item_offset)
    assert np.array_equal(got[1], want_i) and np.array_equal(got[0].view(np.int32), want_v.view(np.int32)), f'{what}: lists differ from the oracle'


def test_reuse_through_scorer_exclusions_holder():
    """ops.ScorerExclusions: the same holder and geometry reuses the buffer; another item_offset, another Bu and the other route each
    rebuild the stream (holder.key changes) and the lists are exact for the new geometry; an empty CSR yields no buffer and unmasked lists."""
    ops = S().ops
    k, I = 10, 200
    base = C.shard_clip(off=300)
    with f16_route(1):
        run = Run(base, 'f16-128')
        holder = ops.ScorerExclusions()
        rk0, rk1 = C.ranks(I, k, 0, 1), C.ranks(I, k, 7, C.stride(I))
        _assert_exact(_ops_call('f16-128', run, k, rk0, holder), base, k, rk0, 'first call')
        p0, key0 = holder.buf.data_ptr(), holder.key
        _assert_exact(_ops_call('f16-128', run, k, rk1, holder), base, k, rk1, 'second call, same geometry')
        assert holder.buf.data_ptr() == p0 and holder.key == key0
        # another item offset: same Bu, I, D and nnz — only the offset tells the two streams apart
        moved = C.reshard(base, 250)
        assert not np.array_equal(C.dense_mask(moved), C.dense_mask(base))
        _assert_exact(_ops_call('f16-128', run, k, rk1, holder, moved), moved, k, rk1, 'another item_offset')
        key1 = holder.key
        assert key1 != key0
        # fewer users
        fewer = C.reshard(base, 250)
        fewer.u_idx, fewer.Bu = base.u_idx[:33], 33
        _assert_exact(_ops_call('f16-128', run, k, rk0, holder, fewer), fewer, k, rk0, 'another Bu')
        key2 = holder.key
        assert key2 not in (key0, key1)
        # the other route (32-item tiles) at the same D
        run32 = Run(base, 'f32s-128')
        _assert_exact(_ops_call('f32s-128', run32, k, rk1, holder, fewer), fewer, k, rk1, 'the other route')
        assert holder.key not in (key0, key1, key2)
        _assert_exact(_ops_call('f32s-128', run32, k, rk0, holder, fewer), fewer, k, rk0, 'the other route, reused')
        # no exclusions at all: no buffer, unmasked lists
        empty = C._case('empty', sp.csr_matrix((45, 1000), dtype=np.int8), np.arange(45), 300, I)
        run_e = Run(base, 'f16-128')
        run_e.ex = _csr_dev(empty.csr)
        h = ops.ScorerExclusions()
        got = _ops_call('f16-128', run_e, k, rk1, h, empty)
        assert h.buf is None and h.key is None
        _assert_exact(got, empty, k, rk1, 'empty CSR')
        assert (got[1] >= 300).all()


class _TableModel:
    """user / item representations from two tables"""

    def __init__(self, users, items):
        self.users, self.items = users, items

    def eval(self):
        return self

    def get_item_representations(self, idx):
        return self.items[idx]

    def get_user_representations(self, idx):
        return self.users[idx]


@pytest.mark.parametrize('scorer', ['fp16_fused', 'fp32_fused'])
def test_reuse_through_the_evaluator(scorer):
    """A split of 70 of 90 users x 200 items at D = 64, scored in chunks of 32 users: the first evaluation builds one holder per
    (route, chunk) in the split's ``_scorer_excl`` cache, the second — other item representations — reuses their buffers, and both
    dumps equal the oracle. Another user list gets holders of its own and lists that are exact for the new users."""
    mod = S()
    n_users, I, D, k = 90, 200, 64, 20
    rng = np.random.default_rng(11)
    dense = rng.random((n_users, I)) < 0.06
    dense[3] = True                                                  # nothing scoreable
    excl = sp.csr_matrix(dense)
    labels = sp.random(n_users, I, density=0.02, random_state=6, format='csr', dtype=np.float32).astype(bool)
    users_a = rng.permutation(n_users)[:70]
    users_a[5] = 3
    users_a = np.unique(users_a)[::-1].copy()
    users_b = np.setdiff1d(np.arange(n_users), users_a[:len(users_a) - 10])[:len(users_a)]
    assert len(users_b) >= 20 and not np.array_equal(np.sort(users_a)[:len(users_b)], users_b)
    view = SimpleNamespace(n_users=n_users, n_items=I, items_in_split=np.arange(I), users_in_split=users_a, n_items_in_split=I,
                           n_users_in_split=len(users_a), user_sampling_matrix=sp.csr_matrix(labels), exclude_data=excl)
    u32, _ = C.operands(I, D, np.arange(I), n_users)
    model = _TableModel(torch.from_numpy(u32).to(DEV), None)

    def dump(rk):
        model.items = torch.from_numpy(C.operands(I, D, rk)[1]).to(DEV)
        ev = mod.FullEvaluator(config=mod.evaluation._Cfg(top_k=(1, 10, k), calculate_std=False), dataset=view)
        loader = type('L', (), {'dataset': view, 'batch_size': 16})()
        out = mod.gather_recommender_algorithm_results(model, loader, ev, None, DEV, scorer=scorer, user_chunk=32)
        users = np.asarray(view.users_in_split)
        assert np.array_equal(out['user_indices'], users) and out['k'] == k
        case = C._case('split', excl, users, 0, I)
        _assert_exact((out['topk_logits'], out['topk_item_indices'].astype(np.int32)), case, k, rk, f'{scorer} evaluation')
        return out

    def holders():
        return {key: h for key, h in view._scorer_excl.items() if key != 'csr'}

    dump(C.ranks(I, k, 0, 1))
    first = holders()
    n_chunks = -(-len(users_a) // 32)
    assert len(first) == n_chunks and all(key[0] == scorer for key in first) and all(h.buf is not None for h in first.values())
    ptrs = {key: h.buf.data_ptr() for key, h in first.items()}
    dump(C.ranks(I, k, 4, C.stride(I)))
    second = holders()
    assert set(second) == set(first) and all(second[key] is first[key] and second[key].buf.data_ptr() == ptrs[key] for key in first)
    view.users_in_split, view.n_users_in_split = users_b, len(users_b)
    dump(C.ranks(I, k, 2, C.stride(I)))
    third = holders()
    assert len(set(third) - set(first)) == -(-len(users_b) // 32), 'the new user list did not get holders of its own'
