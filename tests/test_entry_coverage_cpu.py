"""A ledger of which test reaches which entry point, from text alone (nothing is imported or run): every ``sbr_*`` function declared in
include/sibrar_hip.h is named in some tests/test_*.py module, or stands in REACHED_THROUGH with the Python wrapper through which a
named test module reaches it. For a table row the test checks the chain link by link: the test module names ``names``, the first
wrapper's source names it too, every wrapper's source names the next wrapper, and the last one's source names the entry. An entry that
a new kernel adds without a test, or a wrapper that stops calling its entry, fails here. A second ledger covers the entries that take a
leading dimension (a parameter ``long ld...``): each is named in one of the big-ld modules (tests/test_hip_big_ld.py and its siblings
_gemm and _rows), which run it with row offsets past 2^31 and 2^32 elements, or stands in BIG_LD_EXEMPT with a reason that names the
operand's size, so that a new entry with an ld fails until someone decides. No GPU."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, 'tests')
PACKAGE = os.path.dirname(glob.glob(os.path.join(ROOT, '*', '_lib.py'))[0])

# entry -> (test module, the word it names, [(package file, function or class), ...] from the test's side to the entry's)
_PRODUCER = ('test_hip_pinned.py', '_native', [('datasets.py', '_native_producer'), ('native_loader.py', 'NativeBatchProducer')])
REACHED_THROUGH = {
    'sbr_infonce_max_n': ('test_hip_tail.py', 'infonce_max_n', [('ops.py', 'infonce_max_n')]),
    'sbr_host_assemble_items': ('test_host_cpu.py', 'recbole_negative_collate', [('sampling.py', 'recbole_negative_collate')]),
    'sbr_host_csr_contains': ('test_hip_pinned.py', 'DevicePositiveIndex', [('sampling.py', 'DevicePositiveIndex')]),
    'sbr_host_mt19937_randint': ('test_host_cpu.py', 'legacy_randint', [('sampling.py', 'legacy_randint')]),
    'sbr_producer_create': _PRODUCER, 'sbr_producer_set_entity': _PRODUCER, 'sbr_producer_start': _PRODUCER, 'sbr_producer_next': _PRODUCER,
    'sbr_producer_wait': _PRODUCER, 'sbr_producer_release': _PRODUCER, 'sbr_producer_stop': _PRODUCER, 'sbr_producer_destroy': _PRODUCER,
}
# the dense-block entries that only model fits reached before tests/test_hip_block_edges.py: named there directly, not through a wrapper
NAMED_IN_BLOCK_EDGES = ('sbr_rotate_cols_f32', 'sbr_col_residual_f32', 'sbr_ease_weights_f32')


# the modules that run an entry with an operand at a leading dimension past 2^25 elements (row offsets past 2^31 and 2^32 elements)
BIG_LD_MODULES = ('test_hip_big_ld.py', 'test_hip_big_ld_gemm.py', 'test_hip_big_ld_rows.py')
# entries with a `long ld...` parameter that those modules leave out, each with the size its ld operands can take. A training batch has
# B x (1 + negatives) slots, some 10^5 at the most, and a representation a few hundred columns: 2^31 elements would need millions of slots
_BATCH = ' has one row per training-batch slot and at most 1024 columns: 2^31 elements would need a batch of millions of slots'
_TABLE = ('its dense operands (the similarities, gradients and saved statistics) have one row per training-batch slot and at most a few '
          'hundred columns: 2^31 elements would need a batch of millions. W, the embedding table gathered through `rows`, IS catalogue-sized '
          '(2^31 elements at 33.6 M rows x 64 columns; tile64_f32.h widens rows[j] to long before the multiply by ldw); it is not pinned '
          'yet: the case needs the fused kernel\'s whole reference at a 130-row table and is left to a follow-up')
BIG_LD_EXEMPT = {
    **{e: 'dY, Y and dZ [slots, C]: each' + _BATCH for e in ('sbr_act_grad_gather', 'sbr_act_grad_gather_colsum')},
    'sbr_colsum': 'X [slots, C]: it' + _BATCH,
    **{e: 'A, B (and dA, dB) [G x N slots, D <= 512]: each' + _BATCH for e in (
        'sbr_infonce_fwd', 'sbr_infonce_bwd', 'sbr_infonce_gemm_fwd', 'sbr_infonce_gemm_bwd')},
    **{e: _TABLE for e in ('sbr_proto_sim_fwd', 'sbr_proto_sim_bwd', 'sbr_proto_score_fwd', 'sbr_proto_score_bwd', 'sbr_anchor_mix_fwd',
                           'sbr_anchor_mix_bwd')},
    **{e: 'W and dW [R, D] are the looked-up rows of the batch, not the table (the entry takes no row map): each' + _BATCH for e in (
        'sbr_cluster_affil_fwd', 'sbr_cluster_affil_bwd')},
}


def _read(path):
    with open(path) as fh:
        return fh.read()


def declared():
    text = re.sub(r'/\*.*?\*/', ' ', _read(os.path.join(ROOT, 'include', 'sibrar_hip.h')), flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    return sorted(set(re.findall(r'\b(sbr_\w+)\s*\(', text)))


def _test_modules():
    return {os.path.basename(p): _read(p) for p in sorted(glob.glob(os.path.join(TESTS, 'test_*.py'))) if os.path.abspath(p) != os.path.abspath(__file__)}


def names(text, word):
    return re.search(r'(?<![A-Za-z0-9_])' + re.escape(word) + r'(?![A-Za-z0-9_])', text) is not None


def source_of(file, name):
    text = _read(os.path.join(PACKAGE, file))
    found = [n for n in ast.walk(ast.parse(text)) if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name == name]
    assert len(found) == 1, f'{file}: {len(found)} definitions of {name}'
    return ast.get_source_segment(text, found[0])


def test_every_declared_entry_is_reached_by_a_test():
    entries, mods = declared(), _test_modules()
    assert len(entries) >= 157 and 'sbr_last_error' in entries and all(e.startswith('sbr_') for e in entries)
    unnamed = [e for e in entries if not any(names(text, e) for text in mods.values())]
    unreached = sorted(set(unnamed) - set(REACHED_THROUGH))
    print(f'{len(entries)} entries declared, {len(entries) - len(unnamed)} named in a test module, {len(unnamed)} reached through a wrapper, '
          f'{len(unreached)} reached by nothing')
    assert not unreached, f'declared in include/sibrar_hip.h and reached by no test: {unreached}'
    stale = sorted(e for e in REACHED_THROUGH if e not in entries or e not in unnamed)
    assert not stale, f'rows of REACHED_THROUGH that are not needed (named directly by now, or no longer declared): {stale}'


def test_the_table_rows_hold_link_by_link():
    mods = _test_modules()
    for entry, (module, word, chain) in REACHED_THROUGH.items():
        assert module in mods and names(mods[module], word), f'{entry}: tests/{module} does not name {word}'
        sources = [source_of(file, name) for file, name in chain]
        assert names(sources[0], word), f'{entry}: {chain[0]} does not name {word}'
        for (file, name), src, nxt in zip(chain, sources, chain[1:]):
            assert names(src, nxt[1]), f'{entry}: {file}:{name} does not name {nxt[1]}'
        assert names(sources[-1], entry), f'{entry}: {chain[-1]} does not name the entry'


def entries_with_a_leading_dimension():
    """every declared sbr_* function with a parameter of type ``long`` whose name matches ld\\w*"""
    text = re.sub(r'/\*.*?\*/', ' ', _read(os.path.join(ROOT, 'include', 'sibrar_hip.h')), flags=re.S)
    text = re.sub(r'//[^\n]*', ' ', text)
    found = []
    for name, params in re.findall(r'\b(sbr_\w+)\s*\(([^)]*)\)', text):
        if any(re.fullmatch(r'(?:const\s+)?long\s+ld\w*', p.strip()) for p in params.split(',')):
            found.append(name)
    return sorted(set(found))


def test_every_entry_with_a_leading_dimension_is_pinned_past_2_to_31_or_exempt():
    with_ld = entries_with_a_leading_dimension()
    texts = {m: _read(os.path.join(TESTS, m)) for m in BIG_LD_MODULES}
    named = [e for e in with_ld if any(names(text, f"'{e}'") for text in texts.values())]
    print(f'{len(with_ld)} entries take a leading dimension, {len(named)} named in tests/test_hip_big_ld*.py, {len(BIG_LD_EXEMPT)} exempt')
    assert len(with_ld) >= 61 and 'sbr_gram_dense' in with_ld and 'sbr_topk_rows' in with_ld and 'sbr_splitk_reduce_multi' not in with_ld
    undecided = sorted(set(with_ld) - set(named) - set(BIG_LD_EXEMPT))
    assert not undecided, f'take a leading dimension, and are neither in tests/test_hip_big_ld*.py nor in BIG_LD_EXEMPT: {undecided}'
    stale = sorted(e for e in BIG_LD_EXEMPT if e not in with_ld or e in named)
    assert not stale, f'rows of BIG_LD_EXEMPT that are not needed (named in a module by now, or without a leading dimension): {stale}'
    assert all(reason.strip() for reason in BIG_LD_EXEMPT.values()) and len(BIG_LD_EXEMPT) <= 17
    for m, text in texts.items():
        assert 'pytestmark = pytest.mark.gpu' in text, f'tests/{m} is not marked gpu as a whole'
        assert '_BigLd._flat()' in text and '_BigLd.release()' in text, f'tests/{m} does not own and free the one large buffer'


def test_the_dense_block_entries_are_named_directly():
    text = _read(os.path.join(TESTS, 'test_hip_block_edges.py'))
    for entry in NAMED_IN_BLOCK_EDGES + ('sbr_gram_f32', 'sbr_als_gram_f32', 'sbr_als_solve_rows_f32', 'sbr_tri_solve_rows_f32', 'sbr_chol_f32'):
        assert names(text, f"'{entry}'"), f'tests/test_hip_block_edges.py does not call {entry}'
    assert 'pytestmark = pytest.mark.gpu' in text
