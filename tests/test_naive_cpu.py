"""PopularItems / RandomItems without a GPU: the restatements of tests/naive_ref.py against brute force and against known answers of
Philox4x32-10, the g27 fixture recorded from the reference, and the host side of sibrar_amd.naive — registry, constructors,
build_from_conf, the refusals, the header and the library's exports."""
import ctypes
import importlib
import os
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import naive_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS, META = R.load_g27()


def S():
    import sibrar_amd
    return sibrar_amd


def test_restatement_equals_brute_force():
    rng = np.random.default_rng(0)
    for trial in range(60):
        n, k = int(rng.integers(1, 40)), int(rng.integers(1, 45))
        kind = trial % 4
        score = (rng.integers(0, 4, size=n) if kind < 2 else rng.standard_normal(n)).astype(np.float32)
        if kind == 1:
            score = np.where(score == 0, np.float32(-0.0), score).astype(np.float32)
            score[rng.integers(0, n)] = 0.0                                   # both zeros: one score
        if kind == 3:
            score[rng.integers(0, n)] = -np.inf                               # a real entry with the lowest score
        rows = [np.sort(rng.choice(n, size=int(rng.integers(0, n + 1)), replace=False)) for _ in range(5)]
        rows[0], rows[1] = np.arange(0), np.arange(n)                         # nothing excluded, everything excluded
        indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        indices = np.concatenate(rows).astype(np.int32)
        u_idx = rng.integers(0, 5, size=7)
        val, idx = R.shared_rank_topk_ref(score, u_idx, indptr, indices, k)
        assert val.dtype == np.float32 and idx.dtype == np.int32 and val.shape == idx.shape == (7, k)
        for b, u in enumerate(u_idx):
            want = R.brute_force_topk(score, rows[u], k)
            assert idx[b, :len(want)].tolist() == want, (trial, b)
            assert (idx[b, len(want):] == -1).all() and np.isneginf(val[b, len(want):]).all()
            assert np.array_equal(val[b, :len(want)].view(np.int32), score[want].view(np.int32))
    assert R.stable_order(np.array([0.0, 1.0, -0.0, 1.0, -1.0], dtype=np.float32)).tolist() == [1, 3, 0, 2, 4]


def test_philox_known_answers():
    """Random123's first known-answer vector of philox4x32-10 — zero counter, zero key -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8 — was
    confirmed against rocRAND's host-callable engine (rocrand/rocrand_philox4x32_10.h, compiled as a small host program): the two agree,
    no correction was needed. The other vectors are that engine's answers at the counter layout of sbr_uniform_rows_f32."""
    assert R.KNOWN_ANSWERS[0] == ((0, 0), (0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8))
    for key, counter, want in R.KNOWN_ANSWERS:
        got = R.philox4x32_10(np.array(counter, dtype=np.uint32), key)
        assert got.dtype == np.uint32 and tuple(int(x) for x in got) == want, (key, counter)
    batch = R.philox4x32_10(np.array([c for _, c, _ in R.KNOWN_ANSWERS[1:2]] * 3, dtype=np.uint32), R.KNOWN_ANSWERS[1][0])
    assert batch.shape == (3, 4) and (batch == np.array(R.KNOWN_ANSWERS[1][2], dtype=np.uint32)).all()


def test_uniform_rows_restatement():
    assert R.unit_float(np.array([0, 255, 256, 0xFFFFFFFF], dtype=np.uint32)).tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24]
    rows = R.uniform_rows_ref(3, [7, (1 << 31) + 5, 7], 11)
    assert rows.dtype == np.float32 and rows.shape == (3, 11) and np.array_equal(rows[0], rows[2]) and not np.array_equal(rows[0], rows[1])
    assert np.array_equal(rows[0, 8:11], R.unit_float(np.array(R.KNOWN_ANSWERS[1][2][:3], dtype=np.uint32)))       # seed 3, user 7, block 2
    assert np.array_equal(R.uniform_rows_ref(3, [7], 5)[0], rows[0, :5]) and R.uniform_rows_ref(3, [7], 0).shape == (1, 0)
    hi = R.uniform_rows_ref((1 << 64) - 1, [(1 << 40) + 3], 4)[0]
    assert np.array_equal(hi, R.unit_float(np.array(R.KNOWN_ANSWERS[3][2], dtype=np.uint32)))
    big = R.uniform_rows_ref(0, np.arange(50), 1000)
    assert (big >= 0).all() and (big < 1).all() and abs(float(big.astype(np.float64).mean()) - 0.5) < 5 / np.sqrt(12 * big.size)


def test_g27_fixture_against_the_formula_and_predict():
    inter, pop = ARRAYS['inter'], ARRAYS['pop']
    assert inter.shape == (12, 9) and set(np.unique(inter)) == {0., 1.} and META['model_name'] == 'PopularItems'
    counts = inter.sum(axis=0)
    assert counts.tolist() == META['counts'] and (counts == 0).sum() == 1 and len(set(counts.tolist())) < 9         # an empty column, ties
    assert pop.dtype == np.float64 and np.array_equal(pop, counts / counts.sum())                                  # data/dataset.py:357-359
    u, i, pred = ARRAYS['u_idxs'], ARRAYS['i_idxs'], ARRAYS['predict']
    assert pred.dtype == np.float64 and pred.shape == i.shape == (7, 5) and np.array_equal(pred, pop[i])            # exactly, in float64
    Sm = S()
    m = Sm.PopularItems(pop, device='cpu')
    got = m.predict(torch.from_numpy(u), torch.from_numpy(i))
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), pred.astype(np.float32))                     # after the fp32 cast
    # the fp32 cast keeps every strict order and adds no ties (counts far below 2^23)
    p32 = m.pop_distribution.numpy()
    assert np.array_equal(np.sign(p32[:, None] - p32[None, :]), np.sign(pop[:, None] - pop[None, :]))
    built = Sm.PopularItems.build_from_conf({}, SimpleNamespace(user_sampling_matrix=sp.csr_matrix(inter)))
    assert torch.equal(built.pop_distribution, m.pop_distribution)
    full = m.combine_user_item_representations(m.get_user_representations(torch.tensor([4, 4, 9])), m.get_item_representations(torch.arange(9)))
    assert tuple(full.shape) == (3, 9) and full.is_contiguous() and np.array_equal(full.numpy(), np.tile(p32, (3, 1)))
    some = torch.tensor([8, 2, 2, 5])
    assert torch.equal(m.combine_user_item_representations(torch.tensor([1, 0]), (some,)), full[:2][:, some])


def test_registry_constructors_and_conf(tmp_path):
    Sm = S()
    assert Sm.ALGORITHMS['pop'] is Sm.PopularItems and Sm.ALGORITHMS['rand'] is Sm.RandomItems
    import sibrar_amd
    assert sibrar_amd.PopularItems is Sm.PopularItems and sibrar_amd.RandomItems is Sm.RandomItems
    pop = np.array([0.5, 0.25, 0.25, 0.])
    p = Sm.PopularItems(pop)
    assert (p.name, p.device, p.n_items) == ('PopularItems', torch.device('cuda'), 4) and p.pop_distribution.dtype == torch.float32
    assert p.eval() is p and p.train() is p and p.to('cpu') is p and p.device == torch.device('cpu') and callable(p.topk_lists)
    assert p.save_model_to_path(str(tmp_path)) is None and p.load_model_from_path(str(tmp_path)) is None and not os.listdir(tmp_path)
    assert Sm.PopularItems(torch.tensor(pop)).pop_distribution.tolist() == pop.tolist()
    with_pop = Sm.PopularItems.build_from_conf({'alg': 'pop'}, SimpleNamespace(pop_distribution=pop, user_sampling_matrix=None))
    assert type(with_pop) is Sm.PopularItems and with_pop.pop_distribution.tolist() == pop.tolist()
    x = sp.csr_matrix(np.array([[1, 1, 0, 0], [1, 0, 1, 0]]))
    assert Sm.ALGORITHMS['pop'].build_from_conf({}, SimpleNamespace(user_sampling_matrix=x)).pop_distribution.tolist() == pop.tolist()
    r = Sm.RandomItems()
    assert (r.name, r.seed, r.device) == ('RandomItems', 0, torch.device('cuda')) and not hasattr(r, 'topk_lists')
    assert r.eval() is r and r.train() is r and r.to('cpu') is r
    assert r.save_model_to_path(str(tmp_path)) is None and r.load_model_from_path(str(tmp_path)) is None and not os.listdir(tmp_path)
    assert Sm.RandomItems.build_from_conf({}, None).seed == 0 and Sm.ALGORITHMS['rand'].build_from_conf({'seed': 7}, None).seed == 7
    assert Sm.RandomItems(seed=(1 << 64) - 1).seed == (1 << 64) - 1
    u = r.get_user_representations(torch.tensor([3, 1], dtype=torch.int32))
    i = r.get_item_representations(np.array([2, 0]))
    assert u.dtype == torch.int64 and isinstance(i, tuple) and len(i) == 1 and i[0].dtype == torch.int64


@pytest.mark.parametrize('pop, match', [(np.array([0.5, np.nan]), 'non-finite'), (np.array([0.5, np.inf]), 'non-finite'),
                                        (np.zeros((2, 2)), 'vector'), (np.float64(0.5), 'vector'), (np.array(['a']), 'vector'),
                                        (np.array([1e39]), 'fp32 range')])
def test_popular_items_refusals(pop, match):
    with pytest.raises(ValueError, match=match):
        S().PopularItems(pop)


def test_other_refusals():
    Sm = S()
    with pytest.raises(ValueError, match='non-finite'):                       # nobody interacted with anything: 0 / 0
        Sm.PopularItems.build_from_conf({}, SimpleNamespace(user_sampling_matrix=sp.csr_matrix((3, 4))))
    for seed in (-1, 1 << 64, 0.5, True):
        with pytest.raises(ValueError, match='seed'):
            Sm.RandomItems(seed)
    cpu = torch.zeros(3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Sm.ops.shared_ranking(cpu)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Sm.ops.uniform_rows(0, torch.zeros(3, dtype=torch.int64), 4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Sm.RandomItems(device='cpu').predict(torch.tensor([0]), torch.tensor([[0]]))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Sm.PopularItems(np.ones(3), device='cpu').topk_lists(torch.tensor([0]), torch.arange(3), torch.zeros(2, dtype=torch.int64),
                                                             torch.zeros(0, dtype=torch.int32), 2)


def test_header_declares_and_library_exports_the_entry_points():
    lib = importlib.import_module(S().ops.__name__.rsplit('.', 1)[0] + '._lib')
    protos = lib.parse_header()
    assert protos['sbr_shared_rank_topk'][2] == ['order', 'score', 'n_items', 'u_idx', 'excl_indptr', 'excl_indices', 'Bu', 'k', 'out_val',
                                                 'out_idx', 'stream']
    assert protos['sbr_shared_rank_topk'][1][6:8] == [ctypes.c_long, ctypes.c_int]
    assert protos['sbr_uniform_rows_f32'][2] == ['seed', 'u_idx', 'Bu', 'n_items', 'out', 'ld', 'stream']
    assert protos['sbr_uniform_rows_f32'][1] == [ctypes.c_ulong, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_long,
                                                 ctypes.c_void_p]
    text = open(os.path.join(ROOT, 'include', 'sibrar_hip.h')).read()
    assert 'naive_algs.py:35-60' in text and 'naive_algs.py:11-32' in text and 'Philox4x32-10' in text
    handle = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(handle, 'sbr_shared_rank_topk') and hasattr(handle, 'sbr_uniform_rows_f32') and handle.sbr_abi_version() == 4
    handle.sbr_last_error.restype = ctypes.c_char_p
    # argument checks are host arithmetic: they answer without a device
    topk = handle.sbr_shared_rank_topk
    topk.restype, topk.argtypes = protos['sbr_shared_rank_topk'][:2]
    assert topk(None, None, 5, None, None, None, 0, 3, None, None, None) == 0                     # no users: nothing to do
    for args, word in (((None, None, 5, None, None, None, 0, 0, None, None, None), 'at least 1'),
                       ((None, None, 5, None, None, None, 2, 3, None, None, None), 'null operand'),
                       ((None, None, -1, None, None, None, 2, 3, None, None, None), 'negative size')):
        assert topk(*args) == 1 and word in handle.sbr_last_error().decode(), word
    rows = handle.sbr_uniform_rows_f32
    rows.restype, rows.argtypes = protos['sbr_uniform_rows_f32'][:2]
    assert rows(0, None, 0, 5, None, 5, None) == 0 and rows(0, None, 3, 0, None, 0, None) == 0    # no users / no items
    for args, word in (((0, None, 3, 5, None, 5, None), 'null operand'), ((0, None, -3, 5, None, 5, None), 'negative size')):
        assert rows(*args) == 1 and word in handle.sbr_last_error().decode(), word
