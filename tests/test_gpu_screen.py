"""
Mutant screens over samples (bsx_run_screen_sampled, Engine.screen_sampled) against the exact reference: screen_ref
restates the definition of include/bsx.h over sample_ref and WideRef.  Every comparison is exact equality on integers: per
mutant the whole table (key, length, count, sum of l, sum of l^2) and the number of samples without an attractor.

A range is G + 37 samples from 1000003 (G = 32 L, a group): unaligned, with a ragged second group.  The cases' mutants
(screen_ref.mutants_of) and their non-vacuity (screen_ref.assert_not_vacuous) come from the reference alone.
"""
import contextlib
import ctypes as C
import faulthandler

import numpy as np
import pytest

from boolsi_amd import _lib
from boolsi_amd._lib import ptr
from boolsi_amd.attract import merge_tables

import screen_ref
from screen_ref import CASES, CONSTANT_MUTANTS, FIRST, SEED, compiled, compiled_with, count_of, mutants_of, split_max_t, split_mutants, table_of

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_UNSUPPORTED, ERR_TABLE_FULL, ERR_STATE, ERR_RANGE_TOO_LARGE = -1, -4, -5, -7, -9
TIME_LIMIT_S = 120
INLINE_RECORDS = 256


@pytest.fixture(autouse=True)
def time_limit():
    """A test that hangs in a device wait ends the process with a traceback instead of waiting for ever."""
    faulthandler.dump_traceback_later(TIME_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@contextlib.contextmanager
def engine(monkeypatch, name=None, wide=False, chunk=None):
    """A fresh engine under the given environment (the library reads it at every call), with the case loaded."""
    from boolsi_amd.engine import Engine
    with monkeypatch.context() as mp:
        for var, val in (('BSX_WIDE', '1' if wide else None), ('BSX_WIDE_CHUNK', chunk)):
            if val is None:
                mp.delenv(var, raising=False)
            else:
                mp.setenv(var, str(val))
        eng = Engine(0)
        try:
            if name:
                net, space, _ = compiled(name)
                eng.set_problem(net, space)
            yield eng
        finally:
            eng.close()


def key_words(recs):
    return [tuple(int(w) for w in r['key']) for r in recs]


def check(eng, name, mutants, first=FIRST, count=None, max_t=None, max_len=None, want=None):
    """One screen call against the reference (or `want`: [(table, none)] per mutant) -> stats"""
    count = count_of(name) if count is None else count
    if want is None:
        # (only what differs from the defaults: the reference keeps one result per distinct call)
        kw = {k: v for k, v in (('first', first), ('count', count), ('max_t', max_t), ('max_len', max_len))
              if v is not None and (k, v) not in (('first', FIRST), ('count', count_of(name)))}
        want = [table_of(name, m, **kw) for m in mutants]
    records, none, stats = eng.screen_sampled(SEED, first, count, mutants, max_t if max_t is not None else float('inf'),
                                              max_len if max_len is not None else float('inf'))
    assert len(records) == len(mutants) == len(none)
    for m, (recs, (table, n_none)) in enumerate(zip(records, want)):
        assert merge_tables([recs]) == table, (name, mutants[m])
        assert int(none[m]) == n_none == count - sum(e[1] for e in table.values())
        assert key_words(recs) == sorted(key_words(recs)), 'records of a mutant are not in key order'
    total = sum(len(r) for r in records)
    assert stats['problems'] == len(mutants) * count
    assert stats['host_syncs'] == (2 if total > INLINE_RECORDS else 1)
    assert stats['kernel_launches'] == 2 * stats['dominant_launches'] + 1
    assert 0 < stats['executed_steps']
    return stats


@pytest.mark.parametrize('name', list(CASES))
def test_screen_equals_the_reference(monkeypatch, name):
    screen_ref.assert_not_vacuous(name)
    net = compiled(name)[0]
    mutants = mutants_of(name)
    if name == 'n600_wide_inputs':
        assert sorted(len(p) for p in net.predecessor_lists)[-2:] == [9, 12] and ((123, 1),) in mutants
    with engine(monkeypatch, name) as eng:
        assert eng.wide == (net.n_nodes > 256)
        stats = check(eng, name, mutants)
        assert stats['dominant_launches'] == 1
        if name == 'n1024_many_attractors':
            # more records than come back with the header: the second copy
            assert sum(len(table_of(name, m)[0]) for m in mutants) > INLINE_RECORDS and stats['host_syncs'] == 2


def test_the_suite_is_not_vacuous():
    """Over the cases: a mutant with another number of attractors than the wild type, and a non-empty mutant whose table
    is the wild type's."""
    fewer = same = 0
    for name in CASES:
        wild = table_of(name, ())
        for m in mutants_of(name)[1:]:
            fewer += len(table_of(name, m)[0]) != len(wild[0])
            same += table_of(name, m) == wild
    assert fewer and same
    assert len(table_of('n300', ((0, 0),))[0]) == 1 and len(table_of('n300', ())[0]) == 2


@pytest.mark.parametrize('name', list(CASES))
def test_the_wild_type_is_attract_sampled(monkeypatch, name):
    count = count_of(name)
    with engine(monkeypatch, name) as eng:
        plain = eng.attract_sampled(SEED, FIRST, count)
        records, none, _ = eng.screen_sampled(SEED, FIRST, count, [(), mutants_of(name)[1], ()])
    for m in (0, 2):
        assert records[m].tobytes() == plain.table.tobytes() and len(plain.table) > 0
        assert int(none[m]) == plain.n_no_attractor
    assert records[1].tobytes() != plain.table.tobytes()


@pytest.mark.parametrize('name', list(CONSTANT_MUTANTS))
def test_constant_node_mutants_equal_the_space_that_fixes_them(monkeypatch, name):
    count = count_of(name)
    mutants = CONSTANT_MUTANTS[name]
    with engine(monkeypatch, name) as eng:
        records, none, _ = eng.screen_sampled(SEED, FIRST, count, mutants)
        for m, mutant in enumerate(mutants):
            eng.set_problem(*compiled_with(name, mutant))
            plain = eng.attract_sampled(SEED, FIRST, count)
            assert records[m].tobytes() == plain.table.tobytes() and len(plain.table) > 0, mutant
            assert int(none[m]) == plain.n_no_attractor


def test_per_lane_handle_and_wide_handle_agree(monkeypatch):
    name = 'n64'
    with engine(monkeypatch, name) as eng:
        assert not eng.wide
        lane = eng.screen_sampled(SEED, FIRST, count_of(name), mutants_of(name))
    with engine(monkeypatch, name, wide=True) as eng:
        assert eng.wide
        check(eng, name, mutants_of(name))
        wide = eng.screen_sampled(SEED, FIRST, count_of(name), mutants_of(name))
    assert [r.tobytes() for r in lane[0]] == [r.tobytes() for r in wide[0]] and lane[1].tolist() == wide[1].tolist()


def test_disjoint_ranges_add_up(monkeypatch):
    name, cut = 'n300', 101
    count, mutants = count_of(name), mutants_of(name)
    with engine(monkeypatch, name) as eng:
        a = eng.screen_sampled(SEED, FIRST, cut, mutants)
        b = eng.screen_sampled(SEED, FIRST + cut, count - cut, mutants)
        check(eng, name, mutants, first=FIRST, count=cut)
    for m, mutant in enumerate(mutants):
        table, none = table_of(name, mutant)
        assert merge_tables([a[0][m], b[0][m]]) == table
        assert int(a[1][m]) + int(b[1][m]) == none


@pytest.mark.parametrize('name', ['n64', 'n1024'])
def test_a_chunk_below_a_group_gives_the_same_records(monkeypatch, name):
    """BSX_WIDE_CHUNK = 1 is clamped to one group per launch: one launch per (mutant, group), two groups per mutant."""
    mutants = mutants_of(name)
    with engine(monkeypatch, name, chunk=1) as eng:
        stats = check(eng, name, mutants)
        assert stats['dominant_launches'] == 2 * len(mutants)


@pytest.mark.parametrize('name', list(CASES))
def test_a_splitting_max_t(monkeypatch, name):
    t = split_max_t(name)
    mutants = split_mutants(name)
    found = [sum(1 for r in screen_ref.records(name, m, max_t=t) if r[0]) for m in mutants]
    assert any(0 < f < count_of(name) for f in found)
    with engine(monkeypatch, name) as eng:
        check(eng, name, mutants, max_t=t)


def test_max_len(monkeypatch):
    name = 'n577'
    mutants = split_mutants(name)
    lams = sorted({r[2] for m in mutants for r in screen_ref.records(name, m) if r[0]})
    assert len(lams) >= 2
    max_len = lams[-1] - 1
    kept = [sum(1 for r in screen_ref.records(name, m, max_len=max_len) if r[0]) for m in mutants]
    assert all(0 < k < count_of(name) for k in kept)
    with engine(monkeypatch, name) as eng:
        check(eng, name, mutants, max_len=max_len)


# ---- refusals: every check comes before a launch, and a failing call leaves the arrays alone ---------------------------

PATTERN = 0xA5


def raw_call(eng, first, count, mutants=((),), offsets=True, nodes=True, n_mutants=None, cap=64, table=True, n_out=True,
             max_t=_lib.T_INF, none_len=None):
    """-> (status, error text, arrays untouched) of a direct call with pattern-filled arrays (False: NULL)"""
    offs = np.zeros(len(mutants) + 1, np.uint32)
    offs[1:] = np.cumsum([len(m) for m in mutants])
    flat = np.zeros(max(int(offs[-1]), 1), _lib.FIXED)
    for i, pair in enumerate(p for m in mutants for p in m):
        flat[i] = pair
    if isinstance(offsets, (list, tuple)):
        offs = np.array(offsets, np.uint32)
    n_mutants = len(mutants) if n_mutants is None else n_mutants
    recs = np.frombuffer(bytearray([PATTERN]) * (max(cap, 1) * _lib.SCREEN_REC.itemsize), _lib.SCREEN_REC)
    none = np.full(len(mutants) if none_len is None else none_len, 0xA5A5A5A5A5A5A5A5, np.uint64)
    n = C.c_uint64(0xA5A5)
    rc = eng._lib.bsx_run_screen_sampled(eng._h, SEED, first, count, ptr(offs) if offsets is not False else None,
                                         ptr(flat) if nodes else None, n_mutants, max_t, _lib.T_INF, ptr(recs) if table else None, cap,
                                         C.byref(n) if n_out else None, ptr(none), C.byref(_lib.Stats2()))
    untouched = (bytes(recs.tobytes()) == bytes([PATTERN]) * recs.nbytes and n.value == 0xA5A5
                 and (none == np.uint64(0xA5A5A5A5A5A5A5A5)).all())
    return rc, eng._lib.bsx_last_error(eng._h).decode(), untouched, recs, n.value, none


def test_nothing_set_is_a_state_error(monkeypatch):
    with engine(monkeypatch) as eng:
        rc, _, untouched = raw_call(eng, 0, 10)[:3]
        assert (rc, untouched) == (ERR_STATE, True)


def test_argument_errors(monkeypatch):
    name = 'n257'                   # 257 nodes, node 100 fixed by the origin
    with engine(monkeypatch, name) as eng:
        cases = [
            (dict(first=2 ** 64 - 5, count=10), ERR_INVALID, ['wraps']),
            (dict(table=False), ERR_INVALID, ['null']),
            (dict(n_out=False), ERR_INVALID, ['null']),
            (dict(offsets=False), ERR_INVALID, ['mut_offsets is null']),
            (dict(mutants=((), ((3, 0),)), nodes=False), ERR_INVALID, ['mut_nodes is null']),
            (dict(mutants=((), (), ()), offsets=[0, 2, 1, 2]), ERR_INVALID, ['do not ascend', 'mutant 1']),
            (dict(mutants=((), ()), offsets=[1, 1, 1]), ERR_INVALID, ['start at 0']),
            (dict(mutants=((), ((1, 0), (2, 0), (3, 0), (4, 0), (5, 0)))), ERR_INVALID, ['mutant 1', 'BSX_SCREEN_MAX_NODES']),
            (dict(mutants=((), ((257, 0),))), ERR_INVALID, ['mutant 1', 'node 257']),
            (dict(mutants=(((3, 0), (4, 1), (3, 1)),)), ERR_INVALID, ['mutant 0', 'node 3', 'twice']),
            (dict(mutants=((), (), ((100, 1),))), ERR_INVALID, ['mutant 2', 'node 100', 'fixed by the origin']),
            (dict(mutants=(((3, 2),),)), ERR_INVALID, ['mutant 0', 'node 3', 'value above 1']),
            (dict(n_mutants=0), ERR_INVALID, ['n_mutants']),
            (dict(n_mutants=_lib.SCREEN_MAX_MUTANTS + 1), ERR_INVALID, ['BSX_SCREEN_MAX_MUTANTS']),
            (dict(mutants=((), ()), count=2 ** 39 + 1), ERR_RANGE_TOO_LARGE, ['2^40']),
        ]
        for kw, status, words in cases:
            kw = dict(kw)
            rc, text, untouched = raw_call(eng, kw.pop('first', 0), kw.pop('count', 10), **kw)[:3]
            assert (rc, untouched) == (status, True) and all(w in text for w in words), (kw, rc, text)
        # the largest product that is allowed gets past the checks of the arguments: 2^40 samples of one mutant would run
        # for hours, so the boundary itself is checked on the host unit (tests/test_screen_host.py has the layout)
        rc, _, _, recs, n, none = raw_call(eng, 5, 0, mutants=((), ((3, 1),)))
        assert rc == 0 and n == 0 and none.tolist() == [0, 0]              # n_samples = 0: BSX_OK, zeros written


@pytest.mark.parametrize('name,word', [('n700_variations', 'fixed-node variations'), ('n600_9_inputs', 'fixed-node variations')])
def test_spaces_with_variations_are_refused(monkeypatch, name, word):
    import sampled_cases
    net, space, _ = sampled_cases.compiled(name)
    with engine(monkeypatch) as eng:
        eng.set_problem(net, space)
        rc, text, untouched = raw_call(eng, 0, 10)[:3]
        assert (rc, untouched) == (ERR_UNSUPPORTED, True) and word in text, text


def test_a_schedule_and_perturbation_variations_are_refused(monkeypatch):
    from boolsi_amd.compile import compile_problem
    from boolsi_amd.constants import Mode
    from boolsi_amd.input import parse_input_text
    from sampled_cases import any_case
    for perturbations, word in (({10: {'1': '2'}}, 'schedule'), ({10: {'0?': '3'}}, 'perturbation variations')):
        text = any_case(300, 2, 2, range(0, 40), perturbations=perturbations)
        with engine(monkeypatch) as eng:
            eng.set_problem(*compile_problem(parse_input_text(text, 100000, Mode.SIMULATE)))
            rc, err, untouched = raw_call(eng, 0, 10)[:3]
            assert (rc, untouched) == (ERR_UNSUPPORTED, True) and word in err, err


def test_a_cap_one_below_the_records_is_table_full(monkeypatch):
    name = 'n577'
    mutants = mutants_of(name)[:3]
    total = sum(len(table_of(name, m)[0]) for m in mutants)
    assert total > 3
    with engine(monkeypatch, name) as eng:
        rc, text, untouched = raw_call(eng, FIRST, count_of(name), mutants=mutants, cap=total - 1)[:3]
        assert (rc, untouched) == (ERR_TABLE_FULL, True) and 'capacity' in text
        rc, _, untouched, recs, n, none = raw_call(eng, FIRST, count_of(name), mutants=mutants, cap=total)
        assert rc == 0 and not untouched and n == total
        assert recs['mutant'].tolist() == sorted(recs['mutant'].tolist())
        for m, mutant in enumerate(mutants):
            table, n_none = table_of(name, mutant)
            assert merge_tables([recs['rec'][recs['mutant'] == m]]) == table and int(none[m]) == n_none
