"""
Attract over sampled initial conditions (bsx_run_attract_sampled, bsx_sample_problems) against the exact reference:
sample_ref.sample_indices turns sample numbers into flat problem indices, WideRef.attract runs them, wide_ref.aggregate
folds the records.  Every comparison is exact equality on integers, whole tables including sum l and sum l^2; nothing
here is statistical.

Each case's `expect_*` function builds the expected results from the reference alone and asserts, from the reference
alone, that the case is not vacuous (at least two attractors, a cycle longer than 1, a transient, found and not found
at the splitting cap, two variants, two T_p).  Seeds and caps in sampled_cases.py were chosen on the CPU so that these
hold.  A range is G + 37 samples from 1000003 (G = 32 L, a group): unaligned, with a ragged second group.
"""
import contextlib
import functools

import numpy as np
import pytest

from boolsi_amd import _lib
from boolsi_amd.attract import merge_tables

import sample_ref
from sampled_cases import FIRST, L_OF, SEED, assert_not_vacuous, compiled, expected, records
from test_gpu_wide_reduce import rows
from wide_ref import code_of, words_of

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_UNSUPPORTED, ERR_TABLE_FULL, ERR_STEP_LIMIT, ERR_STATE = -1, -4, -5, -6, -7
GENEROUS = 400


@contextlib.contextmanager
def engine(monkeypatch, name=None, wide=False, host=False, chunk=None, step_limit=None):
    """A fresh engine under the given environment (the library reads it at every call), with the case loaded."""
    from boolsi_amd.engine import Engine
    with monkeypatch.context() as mp:
        for var, val in (('BSX_WIDE', '1' if wide else None), ('BSX_WIDE_HOST_REDUCE', '1' if host else None),
                         ('BSX_WIDE_CHUNK', chunk), ('BSX_WIDE_STEP_LIMIT', step_limit)):
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


def count_of(name):
    return 32 * L_OF[name] + 37


def check(eng, first, count, max_t, recs, max_len=None, syncs=1):
    r = eng.attract_sampled(SEED, first, count, max_t, max_len if max_len is not None else float('inf'))
    table, none, steps = expected(recs)
    assert merge_tables([r.table]) == table
    assert r.n_no_attractor == none
    assert r.stats['problems'] == count and r.stats['state_steps'] == steps and r.stats['host_syncs'] == syncs
    return r


# ---- bsx_sample_problems ---------------------------------------------------------------------------------------------

SCATTERED = [0, 1, 31, 63, 64, 65, FIRST, FIRST + 61, 2 ** 32 + 17, 2 ** 63, 2 ** 64 - 2, 2 ** 64 - 1, 5]


@pytest.mark.parametrize('name', ['n20', 'n300', 'n1024'])
def test_sample_problems(monkeypatch, name):
    net, space, ref = compiled(name)
    n_any, V = len(space.any_nodes), sample_ref.variant_count(space)
    assert n_any == {'n20': 10, 'n300': 40, 'n1024': 1024}[name]
    want_states, want_variants = [], []
    for j, index in zip(SCATTERED, sample_ref.sample_indices(space, SEED, SCATTERED)):
        want_states.append(words_of(code_of(ref.problem(index).init), net.n_words))
        want_variants.append(index >> n_any)
    assert len({tuple(s) for s in want_states}) == len(SCATTERED)
    if V > 1:
        assert len(set(want_variants)) >= 2
    with engine(monkeypatch, name) as eng:
        assert eng.wide == (net.n_nodes > 256)
        states, variants = eng.sample_problems(SEED, SCATTERED)
    assert np.array_equal(states, np.array(want_states, np.uint64))
    assert variants.tolist() == want_variants


# ---- bsx_run_attract_sampled on the wide family ----------------------------------------------------------------------

SPLIT = {'n257': 29, 'n300': 58, 'n577': 29, 'n600_9_inputs': 100, 'n1024': 40, 'n700_variations': 75}


@functools.lru_cache(maxsize=None)
def expect_wide(name):
    net, space, ref = compiled(name)
    count = count_of(name)
    split, generous = records(name, FIRST, count, SPLIT[name]), records(name, FIRST, count, GENEROUS)
    assert_not_vacuous(generous, split)
    idx = sample_ref.sample_indices(space, SEED, range(FIRST, FIRST + count))
    n_any = len(space.any_nodes)
    if name == 'n577':
        assert n_any == 300 and space.fixed.tolist() == [[5, 1]]
    if name == 'n1024':
        assert n_any == 1024
    if name != 'n600_9_inputs':
        assert sum(1 for a in space.any_nodes.tolist() if a > 255) >= (1 if name == 'n257' else 5)
    if name == 'n600_9_inputs':
        assert sorted(len(p) for p in net.predecessor_lists)[-2:] == [9, 12]
    if sample_ref.variant_count(space) > 1:
        assert len({i >> n_any for i in idx}) >= 2
    if name == 'n700_variations':
        assert sample_ref.variant_count(space) == 36
        assert {ref.problem(i).tp for i in idx} == {7, 9}
        # some sample closes its cycle within the cap counted from its T_p but not by t = cap: the cap counts from 0
        assert any(SPLIT[name] < g[4] <= SPLIT[name] + 9 for g in generous if g[0])
    return split, generous


@pytest.mark.parametrize('name', list(SPLIT))
def test_attract_sampled_at_a_splitting_and_a_generous_cap(monkeypatch, name):
    split, generous = expect_wide(name)
    with engine(monkeypatch, name) as eng:
        assert eng.wide
        check(eng, FIRST, count_of(name), SPLIT[name], split)
        check(eng, FIRST, count_of(name), GENEROUS, generous)
        check(eng, FIRST, count_of(name), None, generous)           # max_t = inf: the generous cap cut nothing off
    assert all(r[0] for r in generous)


# ---- more than 256 records: the drain's first 256 come back with the header, the rest in a second copy ---------------

MANY = 'n1024_many_attractors'


@functools.lru_cache(maxsize=None)
def expect_many():
    recs = records(MANY, FIRST, count_of(MANY), GENEROUS)
    assert_not_vacuous(recs)
    assert len(expected(recs)[0]) > 256, 'the table fits the first copy'
    return recs


def test_more_than_256_records_cost_a_second_wait(monkeypatch):
    recs = expect_many()
    with engine(monkeypatch, MANY) as eng:
        r = check(eng, FIRST, count_of(MANY), GENEROUS, recs, syncs=2)
        assert len(r.table) == len(expected(recs)[0]) > 256
        keys = [tuple(k) for k in r.table['key'].tolist()]
        assert keys == sorted(keys)             # one order across the two copies: key words from key[0] up


# ---- handles of the <= 256-node family: the second lowering ----------------------------------------------------------

LANE = {'n64': 13, 'example2': 4}           # splitting caps
LANE_COUNT = 32 * 64 + 37


@functools.lru_cache(maxsize=None)
def expect_lane(name):
    split, generous = records(name, FIRST, LANE_COUNT, LANE[name]), records(name, FIRST, LANE_COUNT, GENEROUS)
    assert_not_vacuous(generous, split)
    return split, generous


@pytest.mark.parametrize('name', list(LANE))
def test_per_lane_handle_and_wide_handle_agree(monkeypatch, name):
    split, generous = expect_lane(name)
    net, space, _ = compiled(name)
    n_enum = min(space.n_problems, 4096)
    with engine(monkeypatch, name) as eng:
        assert not eng.wide
        before = eng.attract2(0, n_enum, GENEROUS)
        lane = [check(eng, FIRST, LANE_COUNT, LANE[name], split), check(eng, FIRST, LANE_COUNT, GENEROUS, generous)]
        after = eng.attract2(0, n_enum, GENEROUS)
        assert merge_tables([after.table]) == merge_tables([before.table]) and after.n_no_attractor == before.n_no_attractor
        # a new space drops the second lowering: the next sampled call lowers again and gives the same table
        eng.set_space(space)
        again = check(eng, FIRST, LANE_COUNT, GENEROUS, generous)
        assert rows(again.table) == rows(lane[1].table)
    with engine(monkeypatch, name, wide=True) as eng:
        assert eng.wide
        wide = [check(eng, FIRST, LANE_COUNT, LANE[name], split), check(eng, FIRST, LANE_COUNT, GENEROUS, generous)]
    for a, b in zip(lane, wide):
        assert rows(a.table) == rows(b.table) and a.n_no_attractor == b.n_no_attractor


# ---- ranges, launches, the host-reduce path, max_len, cap ------------------------------------------------------------

RANGES = 'n577'


@functools.lru_cache(maxsize=None)
def expect_ranges():
    G = 32 * L_OF[RANGES]
    count = 2 * G + 37                      # three launches of at most G samples
    recs = records(RANGES, FIRST, count, GENEROUS)
    assert_not_vacuous(recs)
    lams = sorted({r[2] for r in recs if r[0]})
    max_len = lams[-1] - 1
    short = records(RANGES, FIRST, count, GENEROUS, max_len)
    assert 0 < sum(1 for r in short if r[0]) < len(short) and max_len >= lams[0]
    cuts = [0, 100, G + 5, count]           # three ragged calls, none of them whole groups
    return count, recs, short, max_len, cuts


def test_three_launches_three_calls_and_the_host_path(monkeypatch):
    count, recs, short, max_len, cuts = expect_ranges()
    G = 32 * L_OF[RANGES]
    n_attractors = len(expected(recs)[0])
    with engine(monkeypatch, RANGES, chunk=G) as eng:
        whole = check(eng, FIRST, count, GENEROUS, recs)
        assert whole.stats['dominant_launches'] == 3 and whole.stats['kernel_launches'] == 7
        parts = [eng.attract_sampled(SEED, FIRST + a, b - a, GENEROUS) for a, b in zip(cuts, cuts[1:])]
        assert merge_tables([p.table for p in parts]) == merge_tables([whole.table])
        assert sum(p.stats['state_steps'] for p in parts) == whole.stats['state_steps']
        for (a, b), p in zip(zip(cuts, cuts[1:]), parts):
            assert merge_tables([p.table]) == expected(recs[a:b])[0]
        check(eng, FIRST, count, GENEROUS, short, max_len=max_len)
        # capacity: exactly the number of attractors fits, one less is BSX_ERR_TABLE_FULL
        exact = eng.attract_sampled(SEED, FIRST, count, GENEROUS, cap=n_attractors)
        assert rows(exact.table) == rows(whole.table)
        with pytest.raises(_lib.EngineError) as e:
            eng.attract_sampled(SEED, FIRST, count, GENEROUS, cap=n_attractors - 1)
        assert e.value.status == ERR_TABLE_FULL
        empty = eng.attract_sampled(SEED, FIRST, 0, GENEROUS)
        assert len(empty.table) == 0 and empty.n_no_attractor == 0
    with engine(monkeypatch, RANGES, chunk=G, host=True) as eng:
        host = check(eng, FIRST, count, GENEROUS, recs, syncs=3)
        assert rows(host.table) == rows(whole.table)
        with pytest.raises(_lib.EngineError) as e:
            eng.attract_sampled(SEED, FIRST, count, GENEROUS, cap=n_attractors - 1)
        assert e.value.status == ERR_TABLE_FULL


# ---- refusals --------------------------------------------------------------------------------------------------------

def test_refusals(monkeypatch):
    net, space, _ = compiled('n577')
    assert len(space.any_nodes) == 300
    mask = np.zeros(net.n_words, np.uint64)
    mask[0] = 1 << 5
    with engine(monkeypatch, 'n577') as eng:
        # (1 << 300: a variant number outside the space; the refusal comes before the index is looked at)
        for call in (lambda: eng.attract_wide(0, 64, GENEROUS), lambda: eng.simulate(0, 64, 4), lambda: eng.simulate(1 << 300, 4, 4),
                     lambda: eng.trajectories(0, [0, 1], [2, 2]), lambda: eng.target(0, 64, 10, mask, mask),
                     lambda: eng.target_summary(0, 64, 10, mask, mask, hist_bins=4)):
            with pytest.raises(_lib.EngineError) as e:
                call()
            assert e.value.status == ERR_UNSUPPORTED and "'any' nodes" in str(e.value)
        with pytest.raises(_lib.EngineError) as e:
            eng.attract_sampled(SEED, 2 ** 64 - 10, 10, GENEROUS)           # first + n = 2^64 wraps to 0
        assert e.value.status == ERR_INVALID
        last = eng.attract_sampled(SEED, 2 ** 64 - 11, 10, GENEROUS)      # ... the last range that does not
        assert merge_tables([last.table]) == expected(records('n577', 2 ** 64 - 11, 10, GENEROUS))[0]
    with engine(monkeypatch) as eng:
        table = np.zeros(4, _lib.ATTR_REC2W)
        import ctypes as C
        n_out, none, st = C.c_uint32(), C.c_uint64(), _lib.Stats2()
        rc = eng._lib.bsx_run_attract_sampled(eng._h, SEED, 0, 10, 100, 100, _lib.ptr(table), 4, C.byref(n_out), C.byref(none), C.byref(st))
        assert rc == ERR_STATE
        assert eng._lib.bsx_sample_problems(eng._h, SEED, None, 0, None, None) == ERR_STATE


def test_step_limit_on_a_chaotic_network(monkeypatch):
    """Unbiased K = 3 tables at n = 300 do not close a cycle within 512 steps; with max_t = inf that is the step limit."""
    from boolsi_amd import synth
    from boolsi_amd.compile import compile_problem
    from boolsi_amd.constants import Mode
    from boolsi_amd.input import parse_input_text
    from test_gpu_wide_exact import yaml_of
    from wide_ref import WideRef
    preds, masks = synth.random_network(300, 3, 77)
    net, space = compile_problem(parse_input_text(yaml_of(preds, masks, ['any'] * 300), 100000, Mode.SIMULATE))
    idx = sample_ref.sample_indices(space, SEED, range(8))
    assert not any(r[0] for r in WideRef(net, space).attract(idx, 2100)[0])      # Brent at limit 512 stops by tau = 512
    from boolsi_amd.engine import Engine
    with monkeypatch.context() as mp:
        mp.setenv('BSX_WIDE_STEP_LIMIT', '512')
        eng = Engine(0)
        try:
            eng.set_problem(net, space)
            sentinel = np.full(16, 0xAB, np.uint8).view(np.uint64)[0]
            eng._attr_table2w = np.full(8, 0, _lib.ATTR_REC2W)
            eng._attr_table2w['length'] = sentinel
            with pytest.raises(_lib.EngineError) as e:
                eng.attract_sampled(SEED, 0, 8, cap=8)
            assert e.value.status == ERR_STEP_LIMIT
            assert (eng._attr_table2w['length'] == sentinel).all()          # nothing written
        finally:
            eng.close()
