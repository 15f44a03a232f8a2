"""ECF (ecf) without a GPU: the restatement tests/ecf_ref.py against the G20 fixture of the real reference (fp32 and float64, the bounds
of test_acf_cpu.py), the registry, build_from_conf, the initialisation, the state_dict layout and a reference checkpoint, the
loss-dictionary, the C ABI additions, the range errors, the no-CPU-fallback contract and the tag-matrix helper."""
import ctypes
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import ecf_ref
from golden_util import GOLDEN, I, U, close, host_dataset, load, state_dict, sub, world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(GOLDEN, 'g20_ecf.json')))['cases']
NEW_SYMBOLS = ('sbr_cluster_affil_workspace', 'sbr_cluster_affil_fwd', 'sbr_cluster_affil_bwd')
KEYS = ['clusters', 'user_embed.weight', 'item_embed.weight']
OTHER_KEYS = ['reg_loss', 'cf_loss', 'ind_loss', 'ts_loss']
TOL = dict(rtol=1e-5, atol=1e-6)


def _tag_csr(z):
    return sp.csr_matrix(z['tags/matrix'])


def _dataset(z, with_sampling_matrix=False):
    ds = host_dataset(world(z))
    ds.tag_matrix = _tag_csr(z)
    if with_sampling_matrix:
        ds.sampling_matrix = ds.user_sampling_matrix_train
    return ds


def _dense(z, dtype):
    """the reference's two dense operands: both are fp32 values (sgd_alg.py:905-906), held in ``dtype``"""
    inter = torch.from_numpy(world(z)['inter'].toarray().astype(np.float32)).to(dtype)
    return inter, torch.from_numpy(z['tags/matrix'].astype(np.float32)).to(dtype)


def _params(z, name, dtype, requires_grad=False):
    sd = {k: v.to(dtype) for k, v in state_dict(z, f'{name}/sd/').items() if k != 'interaction_matrix'}
    return {k: v.requires_grad_(True) for k, v in sd.items()} if requires_grad else sd


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_restatement_equals_g20(case, dtype):
    """logits, every loss-dictionary entry, both losses, every gradient of rec_loss + reg_loss under each loss, all-pairs scores and the
    pre_tune / post_tune outputs of both sides of every recorded case."""
    z = load('g20_ecf')
    name, conf = case['name'], case['conf']
    assert bool((z[f'{name}/logits'] == 0).any()) or case['conf']['top_m'] == case['conf']['n_clusters'], 'disjoint masks give exact zeros'
    u, i, labels = z['u'], z['i'], torch.from_numpy(z['labels'])
    inter, tag = _dense(z, dtype)
    for kind in ('bce', 'bpr'):
        sd = _params(z, name, dtype, True)
        logits, other = ecf_ref.forward(sd, conf, inter, tag, u, i)
        close(logits.detach(), z[f'{name}/logits'], what='logits', **TOL)
        assert list(other) == case['other_keys']
        for k, v in other.items():
            close(v.detach(), z[f'{name}/other_{kind}/{k}'], what=f'{kind} {k}', **TOL)
        loss = ecf_ref.rec_loss(kind, logits, labels)
        close(loss.detach(), z[f'{name}/loss_{kind}'], what=f'{kind} loss', **TOL)
        (loss + other['reg_loss']).backward()
        grads = sub(z, f'{name}/grad_{kind}/')
        assert set(grads) == set(sd)
        for k, g in grads.items():
            close(sd[k].grad, g, what=f'{kind} grad {k}', rtol=1e-5, atol=1e-7, norm_rtol=1e-5)
    with torch.no_grad():
        sd = _params(z, name, dtype)
        close(ecf_ref.scores_all(sd, conf, inter, u), z[f'{name}/scores_all'], what='all-pairs scores', **TOL)
        i_pre, u_pre = ecf_ref.pre_tune(sd, conf, inter, u)
        for which, got in (('item', ecf_ref.post_tune(i_pre)), ('user', ecf_ref.post_tune(u_pre))):
            for n in (0, 1):
                close(got[n], z[f'{name}/{which}_pre_tune/{n}'], what=f'{which} pre_tune / post_tune [{n}]', **TOL)


def test_fixture_covers_what_it_says():
    z = load('g20_ecf')
    by = {c['name']: {**ecf_ref.DEFAULTS, **c['conf']} for c in CASES}
    assert list(by) == ['a_default', 'b_weights', 'c_all_ones', 'd_two_clusters']
    a, b, c, d = by.values()
    assert a['embedding_dim'] <= 16 and all(a[k] == ecf_ref.DEFAULTS[k] for k in ('temp_masking', 'temp_tags', 'lam_cf', 'lam_ind', 'lam_ts'))
    weights = [b[k] for k in ('temp_masking', 'temp_tags', 'lam_cf', 'lam_ind', 'lam_ts')]
    assert len(set(weights)) == 5 and not set(weights) & {ecf_ref.DEFAULTS[k] for k in ('temp_masking', 'temp_tags', 'lam_cf', 'lam_ind', 'lam_ts')}
    assert b['n_clusters'] % 4 == 0
    assert c['top_m'] == c['top_n'] == c['n_clusters']
    assert (d['n_clusters'], d['top_m'], d['top_n']) == (2, 1, 1)
    assert all(cs['alg'] == 'ecf' and cs['model_name'] == 'ECF' and cs['other_keys'] == OTHER_KEYS for cs in CASES)
    assert all(cs['keys'] == ['interaction_matrix'] + KEYS for cs in CASES)
    # the conditions the generator asserts, recomputed in float64
    inter, tag = _dense(z, torch.float64)
    tagm = z['tags/matrix']
    assert bool(((tagm != 0).sum(axis=0) >= 1).all()) and len({tuple(col) for col in tagm.T}) == tagm.shape[1]
    assert bool((inter[torch.from_numpy(z['u']).long()].sum(dim=1) >= 1).all())
    for cs in CASES:
        p, sd = by[cs['name']], _params(z, cs['name'], torch.float64)
        close(z[f'{cs["name"]}/sd/interaction_matrix'], inter, what='interaction_matrix entry', rtol=0, atol=0, norm_rtol=0)
        x_tildes, xs = ecf_ref.items(sd, cs['conf'])
        a_tilde, _ = ecf_ref.users(sd, cs['conf'], inter, z['u'], x_tildes)
        log_b_c = torch.log_softmax((xs.T @ tag) / p['temp_tags'], dim=-1)
        assert float(ecf_ref.gap(x_tildes, p['top_m']).min()) >= 1e-4 and float(ecf_ref.gap(a_tilde, p['top_n']).min()) >= 1e-4
        assert float(ecf_ref.gap(log_b_c, p['top_p']).min()) >= 1e-5


def test_ecf_is_registered():
    import sibrar_amd as S
    assert S.ALGORITHMS['ecf'] is S.ECF
    assert issubclass(S.ECF, S.PrototypeWrapper) and issubclass(S.ECF, S.SGDBasedRecommenderAlgorithm)
    assert not hasattr(S.ECF, 'post_val') and not hasattr(S.ECF, 'fused_score_transform')


def test_build_from_conf_defaults_merging_and_the_sampling_matrix_fallback():
    import sibrar_amd as S
    z = load('g20_ecf')
    m = S.ALGORITHMS['ecf'].build_from_conf({}, _dataset(z))           # every key has the constructor's default (sgd_alg.py:1113-1117)
    got = {k: getattr(m, k) for k in ecf_ref.DEFAULTS}
    assert got == ecf_ref.DEFAULTS and m.name == 'ECF'
    conf = dict(embedding_dim=12, n_clusters=8, top_n=3, top_m=5, temp_masking=1.5, temp_tags=0.5, top_p=2, lam_cf=0.1, lam_ind=0.2, lam_ts=0.3)
    m = S.ECF.build_from_conf({**conf, 'not_a_parameter': 1}, _dataset(z))
    assert {k: getattr(m, k) for k in conf} == conf
    assert tuple(m.clusters.shape) == (8, 12) and tuple(m.user_embed.weight.shape) == (U, 12) and tuple(m.item_embed.weight.shape) == (I, 12)
    # resident CSR on both sides, the tag matrix transposed; nothing dense
    inter = world(z)['inter']
    assert m.interaction_matrix.shape == (U, I) and m.tag_matrix_t.shape == (int(z['tags/n_tags']), I)
    assert m.interaction_matrix.indices.numel() == inter.nnz and m.tag_matrix_t.indices.numel() == _tag_csr(z).nnz
    # dataset.sampling_matrix wins when the dataset has one; otherwise user_sampling_matrix_train
    ds = _dataset(z)
    ds.sampling_matrix = sp.csr_matrix(([1.], ([3], [5])), shape=(U, I))
    m2 = S.ECF.build_from_conf(conf, ds)
    assert m2.interaction_matrix.indices.tolist() == [5] and int(m2.interaction_matrix.indptr[-1]) == 1
    for meth in ('get_user_representations_pre_tune', 'get_user_representations_post_tune', 'get_item_representations_pre_tune',
                 'get_item_representations_post_tune', 'get_and_reset_other_loss'):
        assert callable(getattr(m, meth))
    with pytest.raises(ValueError, match='do not fit'):
        S.ECF(U + 1, I, _tag_csr(z), inter)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_initialisation_with_the_generator_seed_equals_the_fixture(case):
    """user_embed, item_embed (N(0, 1) each), then randperm for the clusters: the reference's RNG order, bit for bit"""
    import sibrar_amd as S
    z = load('g20_ecf')
    torch.manual_seed(case['seed'])
    m = S.ALGORITHMS['ecf'].build_from_conf(case['conf'], _dataset(z, with_sampling_matrix=True))
    sd = state_dict(z, f'{case["name"]}/sd/')
    assert list(m.state_dict().keys()) == KEYS
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert m.clusters.requires_grad and m.clusters.data_ptr() != m.item_embed.weight.data_ptr()


@pytest.mark.parametrize('case', CASES[:2], ids=lambda c: c['name'])
def test_state_dict_keys_and_a_reference_checkpoint(case, tmp_path):
    import sibrar_amd as S
    z = load('g20_ecf')
    m = S.ALGORITHMS['ecf'].build_from_conf(case['conf'], _dataset(z))
    sd = state_dict(z, f'{case["name"]}/sd/')
    assert list(sd) == ['interaction_matrix'] + KEYS and list(m.state_dict().keys()) == KEYS
    m.load_state_dict(sd, strict=True)                        # the reference's interaction_matrix entry is accepted and dropped
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    torch.save(sd, os.path.join(tmp_path, 'model.pth'))
    m2 = S.ECF.build_from_conf(case['conf'], _dataset(z))
    m2.load_model_from_path(str(tmp_path))
    assert all(torch.equal(v, sd[k]) for k, v in m2.state_dict().items())
    with pytest.raises(RuntimeError, match='Unexpected key'):
        m.load_state_dict({**sd, 'something_else': torch.zeros(1)}, strict=True)


def test_other_loss_keys_and_reset_without_a_forward():
    import sibrar_amd as S
    z = load('g20_ecf')
    m = S.ECF.build_from_conf(dict(embedding_dim=4, n_clusters=4, lam_cf=0.5, lam_ind=0.25, lam_ts=2.), _dataset(z))
    assert m.get_and_reset_other_loss() == {'reg_loss': 0., 'cf_loss': 0., 'ind_loss': 0., 'ts_loss': 0.}
    m._acc_cf, m._acc_ind, m._acc_ts = torch.tensor(2.), torch.tensor(4.), torch.tensor(8.)
    out = m.get_and_reset_other_loss()
    assert list(out) == OTHER_KEYS and [float(v) for v in out.values()] == [18., 1., 1., 16.]
    assert m._acc_cf == 0 and m._acc_ind == 0 and m._acc_ts == 0


def test_new_symbols_declared_and_exported():
    import sibrar_amd as S
    from importlib import import_module
    protos = import_module(S.ops.__name__.rsplit('.', 1)[0] + '._lib').parse_header()
    handle = ctypes.CDLL(S.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in protos, f'{name} is not declared in include/sibrar_hip.h'
        assert hasattr(handle, name), f'{name} is not exported by the library'
    assert S.lib().sbr_abi_version() == 4
    header = open(os.path.join(ROOT, 'include', 'sibrar_hip.h')).read()
    assert 'sgd_alg.py:1020-1037' in header and 'sgd_alg.py:988-1009' in header and 'sgd_alg.py:891-1138' in header
    assert 'TIE RULE: equal logits at the mask boundary go to the LOWEST cluster index' in header
    # the workspace sizes are host arithmetic: the reference defaults, and shapes outside the range
    ws = S.lib().sbr_cluster_affil_workspace
    assert ws(45056, 100, 64, 0) > 0 and ws(45056, 100, 64, 1) > ws(45056, 100, 64, 0)
    assert ws(1, 1, 2, 1) > 0 and ws(1, 512, 256, 1) > 0
    for D, C in ((0, 64), (513, 64), (100, 1), (100, 257)):
        assert ws(64, D, C, 0) == 0 and ws(64, D, C, 1) == 0
    assert ws(0, 100, 64, 0) == 0


def test_shapes_outside_the_kernel_range_raise_value_error_before_any_launch():
    import sibrar_amd as S
    ops = S.ops
    for fn in (ops.ClusterAffilFn.apply, ops.cluster_affil):               # checked before anything else: no device needed
        for D, C, top, temp, what in ((513, 20, 2, 2., 'embedding_dim'), (100, 1, 1, 2., 'n_clusters'), (100, 257, 2, 2., 'n_clusters'),
                                      (100, 20, 0, 2., 'top'), (100, 20, 21, 2., 'top'), (100, 20, 2, 0., 'temp'), (100, 20, 2, -1., 'temp')):
            with pytest.raises(ValueError, match=what):
                fn(torch.zeros(3, D), torch.zeros(C, D), None, top, temp)
            if what != 'embedding_dim':
                with pytest.raises(ValueError, match=what):
                    fn(None, None, torch.zeros(3, C), top, temp)
        with pytest.raises(ValueError, match='one width'):
            fn(torch.zeros(3, 8), torch.zeros(4, 9), None, 2, 2.)
        with pytest.raises(ValueError, match='logits alone'):
            fn(torch.zeros(3, 8), None, torch.zeros(3, 4), 2, 2.)
        with pytest.raises(ValueError, match='top'):
            fn(None, None, torch.zeros(3, 4), 2.5, 2.)


def test_cpu_tensors_raise():
    import sibrar_amd as S
    z = load('g20_ecf')
    u, i = torch.zeros(2, dtype=torch.long), torch.zeros(2, 3, dtype=torch.long)
    m = S.ECF.build_from_conf(CASES[0]['conf'], _dataset(z))
    with pytest.raises(RuntimeError, match='CUDA'):
        m(u, i)
    for fn, arg in ((m.get_user_representations, u), (m.get_item_representations, i), (m.get_user_representations_pre_tune, u),
                    (m.get_item_representations_pre_tune, i)):
        with pytest.raises(RuntimeError, match='CUDA'):
            fn(arg)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.ops.ClusterAffilFn.apply(torch.randn(5, 4), torch.randn(3, 4), None, 2, 2.)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.ops.ClusterAffilFn.apply(None, None, torch.randn(5, 4), 2, 2.)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.ops.cluster_affil(torch.randn(5, 4), torch.randn(3, 4), None, 2, 2.)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        S.ops.cluster_affil(None, None, torch.randn(5, 4), 2, 2.)


def test_ecf_tag_matrix_equals_the_reference_matrix():
    import sibrar_amd as S
    z = load('g20_ecf')
    got = S.ecf_tag_matrix(I, z['tags/item_idx'], z['tags/tag_idx'], int(z['tags/n_tags']))
    assert sp.isspmatrix_csr(got) and got.shape == (I, int(z['tags/n_tags'])) and got.dtype == np.float64
    assert np.array_equal(got.toarray(), z['tags/matrix'])
    assert np.array_equal(ecf_ref.tag_matrix(I, z['tags/item_idx'], z['tags/tag_idx'], int(z['tags/n_tags'])), z['tags/matrix'])
    # duplicate pairs add up before the weighting, as np.ones summed by csr_matrix does in the reference
    dup = S.ecf_tag_matrix(3, [0, 0, 1], [0, 0, 1], 2).toarray()
    assert np.allclose(dup, [[2 * np.log(3 / (2 + 1e-6)), 0.], [0., np.log(3 / (1 + 1e-6))], [0., 0.]])


def test_the_restatement_breaks_ties_towards_the_lowest_index():
    t = torch.tensor([[1., 1., 1., 0.], [0., 2., 2., 2.], [-1., -1., 3., -1.]])
    assert ecf_ref.top_mask(t, 2).tolist() == [[1., 1., 0., 0.], [0., 1., 1., 0.], [1., 0., 1., 0.]]
    x = ecf_ref.affiliation(t, 2, 2.)
    assert bool((x[ecf_ref.top_mask(t, 2) == 0] == 0).all()), 'exactly 0 off the mask'
