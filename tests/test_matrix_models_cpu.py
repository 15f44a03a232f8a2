"""The base of the fit(matrix) models (sibrar_amd.matrix_models) without a GPU: a toy model whose score rows are a fixed table on the host
goes through the hooks, predict, attach and model.npz as ResidentMatrixAlgorithm writes them once; and UserKNN, ItemKNN, EASE and P3alpha
stand on that base without a copy of their own; the model.npz fields of the row autoencoders (row_autoencoder.py) round-trip on the host."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch


def S():
    import sibrar_amd
    return sibrar_amd


TABLE = (torch.arange(35.).reshape(5, 7) * 0.37).sin()                           # the toy's score rows: float32 [5 users, 7 items]
U = torch.tensor([3, 0, 3, 4])


def toy(name='Toy'):
    class Toy(S().ResidentMatrixAlgorithm):
        KEY, WHAT, STORES = 'T', 'table', 'the toy table'
        BINARY_ONLY = 'Toy: a toy counts its 0/1 entries'

        def __init__(self):
            super().__init__('cpu')
            self.T = None
            self.name = name

        def fit(self, matrix, **kwargs):
            self.attach(matrix)
            self.T = TABLE.clone()
            return self

        def _score_rows(self, u):
            return self.T[u]

        def _npz_fields(self):
            return {'T': self.T.numpy()}

        def _read_npz(self, f):
            self.T = torch.from_numpy(f['T'])

        @staticmethod
        def build_from_conf(conf, dataset=None):
            return Toy()
    return Toy()


def fitted():
    return toy().fit(sp.csr_matrix(np.ones((5, 7))))


def _combine(m, u, items):
    return m.combine_user_item_representations(m.get_user_representations(u), m.get_item_representations(items))


def test_combine_and_predict_select_from_the_score_rows():
    m = fitted()
    assert TABLE.dtype == torch.float32 and (m.n_users, m.n_items, m.device) == (5, 7, torch.device('cpu'))
    rows = _combine(m, U, torch.arange(7))
    assert rows.dtype == torch.float32 and torch.equal(rows, TABLE[U])             # the identity item list: the very rows
    some = torch.tensor([5, 0, 2])
    assert torch.equal(_combine(m, U, some), TABLE[U][:, some])                     # a permuted 1-D subset
    assert torch.equal(_combine(m, U, torch.arange(7).flip(0)), TABLE[U].flip(1))   # all the items, but not in their order
    items = torch.tensor([[6, 6, 1], [0, 3, 2], [4, 5, 6], [2, 1, 0]])
    want = torch.gather(TABLE[U], 1, items)
    assert torch.equal(_combine(m, U, items), want)                                 # a 2-D item matrix: one list per user
    assert torch.equal(m.predict(U, items), want)
    assert torch.equal(m.predict(U.numpy(), items.numpy()), want)                   # whatever as_tensor takes
    assert not m.predict(U, items).requires_grad and m.to('cpu') is m


def test_attach_refuses_with_the_models_own_sentence():
    dup = sp.coo_matrix((np.ones(3), ([0, 0, 1], [1, 1, 0])), shape=(2, 2))          # a duplicate entry sums to 2
    for bad in (sp.csr_matrix(np.array([[1., 2.], [0., 1.]])), dup):
        with pytest.raises(ValueError, match='Toy: a toy counts its 0/1 entries: the matrix has entries other than 1'):
            toy().attach(bad)
    m = toy().attach(sp.csr_matrix(np.array([[1., 0., 1.], [0., 0., 0.]])))          # explicit zeros and empty rows are fine
    assert (m.n_users, m.n_items) == (2, 3) and m.T is None


def test_state_errors():
    m = toy()
    for use in (lambda: m.predict(U, torch.zeros(4, 1, dtype=torch.long)), lambda: _combine(m, U, torch.arange(7)),
                lambda: m.save_model_to_path('.')):
        with pytest.raises(RuntimeError, match='Toy: no table, run fit'):
            use()
    m.T = TABLE
    with pytest.raises(RuntimeError, match='the table were loaded from model.npz.*attach'):
        m.predict(U, torch.zeros(4, 1, dtype=torch.long))


def test_model_npz(tmp_path, capsys):
    fitted().save_model_to_path(str(tmp_path))
    assert capsys.readouterr().out == 'Model Saved\n'
    with np.load(tmp_path / 'model.npz', allow_pickle=False) as f:
        assert set(f.files) == {'T', 'name'} and str(f['name']) == 'Toy'
    back = toy()
    back.load_model_from_path(str(tmp_path))
    assert capsys.readouterr().out == 'Model Loaded\n'
    assert torch.equal(back.T, TABLE) and back.n_items is None
    with pytest.raises(RuntimeError, match='attach'):
        back.predict(U, torch.zeros(4, 1, dtype=torch.long))                        # the file does not hold the interactions
    other = toy()
    other.load_model_from_path(str(tmp_path), matrix=sp.csr_matrix(np.ones((5, 7))))  # matrix=: attached at once
    assert (other.n_users, other.n_items) == (5, 7) and torch.equal(_combine(other, U, torch.arange(7)), TABLE[U])
    wrong = toy('Other')
    with pytest.raises(ValueError, match='model.npz holds a Toy, this model is a Other'):
        wrong.load_model_from_path(str(tmp_path))
    assert wrong.T is None


def test_foreign_model_files_are_refused(tmp_path):
    np.savez(tmp_path / 'model.npz', pred_mtx=np.zeros((2, 2)))
    with pytest.raises(ValueError, match='pred_mtx.*this package the toy table'):
        toy().load_model_from_path(str(tmp_path))
    np.savez(tmp_path / 'model.npz', pred_mtx=np.zeros((2, 2)), T=TABLE.numpy(), name=np.array('Toy'))
    with pytest.raises(ValueError, match='is not a model of this package'):
        toy().load_model_from_path(str(tmp_path))
    np.savez(tmp_path / 'model.npz', B=np.zeros((2, 2)), name=np.array('Toy'))       # the model's own array is missing
    with pytest.raises(ValueError, match='is not a model of this package'):
        toy().load_model_from_path(str(tmp_path))


def test_row_autoencoder_fields_round_trip(tmp_path):
    """RowAutoencoder's field logic alone, on the host: ``_npz_fields`` -> ``np.savez`` -> ``_read_npz`` on models whose arrays were set by
    hand; None -> NaN -> None for RecVAE's ``gamma`` and ``beta``; a missing key and a wrong shape refused, the model left as it was."""
    Sm = S()
    I, H, L = 7, 4, 3

    def by_hand(cls):
        return {k: torch.arange(float(np.prod(s))).reshape(s) * 0.01 + n for n, (k, s) in enumerate(cls.shapes(I, H, L).items())}

    for cls, kw in ((Sm.RecVAE, dict(gamma=None, beta=0.25)), (Sm.RecVAE, dict(gamma=0.02, beta=None)), (Sm.MultVAE, dict(anneal_cap=0.5)),
                    (Sm.MultDAE, dict(total_anneal_steps=9))):
        m = cls(hidden=H, latent=L, dropout=0.25, lr=3e-3, batch_size=7, n_epochs=2, weight_decay=1e-4, seed=8, device='cpu', **kw)
        arrays = by_hand(cls)
        m._set_weights(arrays)
        fields = m._npz_fields()
        assert set(fields) == set(arrays) | set(cls.HYPER)
        for h in cls.OPTIONAL:
            assert np.isnan(fields[h]) == (getattr(m, h) is None)
        np.savez(tmp_path / 'model.npz', **fields)
        back = cls(device='cpu')
        with np.load(tmp_path / 'model.npz', allow_pickle=False) as f:
            back._read_npz(f)
        for h in cls.HYPER:
            assert getattr(back, h) == getattr(m, h) and type(getattr(back, h)) is type(getattr(m, h)), h
        for part, names in cls.PARTS.items():
            for k in names:
                assert torch.equal(getattr(getattr(back, part), k).detach(), arrays[k]), k
        assert getattr(getattr(back, next(iter(cls.PARTS))), cls.INPUT).t().is_contiguous()
        for drop in (cls.INPUT, 'seed', cls.HYPER[-2]):
            np.savez(tmp_path / 'less.npz', **{k: v for k, v in fields.items() if k != drop})
            fresh = cls(device='cpu')
            with np.load(tmp_path / 'less.npz', allow_pickle=False) as f, pytest.raises(ValueError, match=f"model.npz: no \\['{drop}'\\]"):
                fresh._read_npz(f)
            assert getattr(fresh, cls.KEY) is None and fresh.hidden == 600
        for k in (cls.INPUT, next(reversed(arrays))):
            np.savez(tmp_path / 'bad.npz', **{**fields, k: fields[k][:-1]})
            fresh = cls(device='cpu')
            with np.load(tmp_path / 'bad.npz', allow_pickle=False) as f, pytest.raises(ValueError, match=f'do not belong to a {cls.__name__} with hidden={H}'):
                fresh._read_npz(f)
            assert getattr(fresh, cls.KEY) is None and fresh.hidden == 600


def test_the_four_models_stand_on_the_base():
    Sm = S()
    shared = ('get_user_representations', 'get_item_representations', 'combine_user_item_representations', 'predict', 'attach', '_need_fit',
              'save_model_to_path', 'load_model_from_path')
    for cls in (Sm.UserKNN, Sm.ItemKNN, Sm.EASE, Sm.P3alpha):
        assert issubclass(cls, Sm.ResidentMatrixAlgorithm) and issubclass(Sm.ResidentMatrixAlgorithm, Sm.SparseMatrixBasedRecommenderAlgorithm)
        for c in cls.__mro__[:cls.__mro__.index(Sm.ResidentMatrixAlgorithm)]:          # the model and every layer above the base
            for name in shared:
                assert name not in vars(c), f'{c.__name__} has its own {name}'
    for cls in (Sm.EASE, Sm.P3alpha):
        assert 'to' not in vars(cls) and '_read_npz' not in vars(cls) and '_npz_fields' not in vars(cls)
    assert Sm.knn.SparseMatrixBasedRecommenderAlgorithm is Sm.SparseMatrixBasedRecommenderAlgorithm
    assert Sm.knn._binary_csr is Sm.matrix_models._binary_csr
