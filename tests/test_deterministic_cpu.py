"""No GPU needed: the deterministic mode's switch through the layers — header, exported symbols, flag and counter on the host,
``ops.set_deterministic`` / ``is_deterministic``, ``reproducible``, the ``FusedTrainStep`` / ``Trainer`` parameters and their defaults."""
import ctypes
import inspect
import os
import random
from importlib import import_module

import numpy as np
import torch


def _lib():
    return import_module('sibrar---single-branch-recommender_amd._lib')


def S():
    import sibrar_amd
    return sibrar_amd


def _handle():
    _l = _lib()
    if not os.path.exists(_l.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _l.lib()


def test_deterministic_prototypes_parse_and_are_exported():
    protos = _lib().parse_header()
    vp, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert protos['sbr_set_deterministic'] == (i, [i], ['on'])
    assert protos['sbr_get_deterministic'] == (i, [], [])
    assert protos['sbr_nondeterministic_launches'] == (l, [], [])
    assert protos['sbr_reset_nondeterministic_launches'] == (i, [], [])
    # the fixed-order form takes the argument list of the entry point it stands in for
    assert protos['sbr_scatter_add_rows_det'][1:] == protos['sbr_scatter_add_rows'][1:]
    h = _handle()
    for name in ('sbr_set_deterministic', 'sbr_get_deterministic', 'sbr_nondeterministic_launches',
                 'sbr_reset_nondeterministic_launches', 'sbr_scatter_add_rows_det'):
        assert hasattr(h, name), name
    assert h.sbr_abi_version() == 4
    # the reference call site is named where the entries are declared, like every other entry
    text = open(_lib().HEADER_PATH).read()
    at = text.index('int sbr_set_deterministic')
    assert 'utilities/utils.py:22-27' in text[at - 1500:at]


def test_flag_and_counter_on_the_host():
    h = _handle()
    ops = S().ops
    prev = ops.set_deterministic(False)
    try:
        assert h.sbr_get_deterministic() == 0 and ops.is_deterministic() is False
        assert ops.set_deterministic(True) is False
        assert h.sbr_get_deterministic() == 1 and ops.is_deterministic() is True
        assert ops.set_deterministic(False) is True
        assert h.sbr_get_deterministic() == 0 and ops.is_deterministic() is False
        h.sbr_reset_nondeterministic_launches()
        assert h.sbr_nondeterministic_launches() == 0 and ops.nondeterministic_launches() == 0
        # an entry point without a fixed-order form refuses before it touches the device, and names itself
        ops.set_deterministic(True)
        rc = h.sbr_bias_score_bwd(1, None, None, None, None, None, 1, 1, None)     # g = a non-null dummy; nothing is launched
        assert rc != 0 and b'sbr_bias_score_bwd: no deterministic form' in h.sbr_last_error()
        assert h.sbr_nondeterministic_launches() == 0
    finally:
        ops.set_deterministic(prev)


def test_python_surface_and_defaults(monkeypatch):
    s = S()
    assert s.reproducible is import_module('sibrar---single-branch-recommender_amd').reproducible
    sig = inspect.signature(s.FusedTrainStep.__init__)
    assert 'deterministic' in sig.parameters and sig.parameters['deterministic'].default is None
    assert inspect.signature(s.reproducible).parameters['deterministic'].default is True
    src = inspect.getsource(s.Trainer.__init__)
    assert "_get(conf, 'deterministic', None)" in src
    prev = s.ops.set_deterministic(False)
    try:
        s.reproducible(7)
        assert s.ops.is_deterministic()
        a = (random.random(), float(np.random.rand()), float(torch.rand(1)))
        s.reproducible(7)
        b = (random.random(), float(np.random.rand()), float(torch.rand(1)))
        assert a == b
        s.reproducible(7, deterministic=False)
        assert not s.ops.is_deterministic()
        # the env default, in the style of SBR_GRAPH: read when the mode is first asked for
        monkeypatch.setenv('SBR_DETERMINISTIC', '1')
        monkeypatch.setattr(s.ops, '_DET', None)
        assert s.ops.is_deterministic() and _handle().sbr_get_deterministic() == 1
    finally:
        s.ops.set_deterministic(prev)
