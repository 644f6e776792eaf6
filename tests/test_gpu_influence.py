"""
The influence matrix over samples (bsx_run_influence_sampled) against the exact reference: influence_ref restates the
definition of include/bsx.h over sample_ref and damage_ref.step.  Every comparison is exact equality on integers: the whole
table and the merged counts, for every source and t.

influence_cases.expect builds the expected arrays from the reference alone and asserts, from the reference alone, that a
case is not vacuous.  A range is G + 37 samples from 1000003 (G = 32 L, a group): unaligned, with a ragged second group.
"""
import contextlib
import ctypes as C
import faulthandler

import numpy as np
import pytest

from boolsi_amd import _lib
from boolsi_amd._lib import ptr

import influence_cases
from influence_cases import CASES, FIRST, L_OF, SEED, T, compiled, count_of, expect, sources_of

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_UNSUPPORTED, ERR_STATE, ERR_RANGE_TOO_LARGE = -1, -4, -7, -9
TIME_LIMIT_S = 120


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


def problem_of(text):
    from boolsi_amd.compile import compile_problem
    from boolsi_amd.constants import Mode
    from boolsi_amd.input import parse_input_text
    return compile_problem(parse_input_text(text, 100000, Mode.SIMULATE))


def check_stats(stats, n_sources, count, steps):
    assert stats['problems'] == n_sources * count and stats['state_steps'] == 2 * n_sources * count * steps
    assert 0 < stats['executed_steps'] <= stats['state_steps']


def check(eng, name):
    """The whole call of a case against the reference, with and without the merged counts -> stats"""
    want, want_merged = expect(name)
    sources, count = sources_of(name), count_of(name)
    got, merged, stats = eng.influence_sampled(SEED, FIRST, count, sources, T)
    assert got.dtype == np.uint32 and got.shape == want.shape and merged.dtype == np.uint64 and merged.shape == want_merged.shape
    assert np.array_equal(got, want)
    assert np.array_equal(merged, want_merged)
    check_stats(stats, len(sources), count, T)
    plain, none, _ = eng.influence_sampled(SEED, FIRST, count, sources, T, merged=False)
    assert none is None and np.array_equal(plain, want)
    return stats


@pytest.mark.parametrize('name', list(CASES))
def test_influence_equals_the_reference(monkeypatch, name):
    net = compiled(name)[0]
    if name == 'n600_wide_inputs':
        assert sorted(len(p) for p in net.predecessor_lists)[-2:] == [9, 12]
    with engine(monkeypatch, name) as eng:
        assert eng.wide == (net.n_nodes > 256)
        stats = check(eng, name)
        assert stats['kernel_launches'] == 1
        # groups that have merged stop: fewer updates ran than the definition counts
        assert stats['executed_steps'] < stats['state_steps']


def ring_of_copies(n):
    from test_gpu_wide_exact import yaml_of
    return yaml_of([[(i - 1) % n] for i in range(n)], [0b10] * n, ['any'] * n)


def test_a_ring_of_copies_moves_the_flip_one_node_per_step(monkeypatch):
    """Node i copies node i - 1: source v at time t is exactly N at target (v + t) mod n, 0 elsewhere, and nothing merges."""
    n, count, steps = 300, 32 * 16 + 37, 7
    sources = [0, 1, 150, 296, 299]
    with engine(monkeypatch) as eng:
        eng.set_problem(*problem_of(ring_of_copies(n)))
        got, merged, stats = eng.influence_sampled(SEED, FIRST, count, sources, steps)
    want = np.zeros((len(sources), steps, n), np.uint32)
    for s, v in enumerate(sources):
        for t in range(1, steps + 1):
            want[s, t - 1, (v + t) % n] = count
    assert np.array_equal(got, want) and not merged.any()
    assert stats['executed_steps'] == stats['state_steps'] == 2 * len(sources) * count * steps


def test_per_lane_handle_and_wide_handle_agree(monkeypatch):
    with engine(monkeypatch, 'n64') as eng:
        assert not eng.wide
        lane = eng.influence_sampled(SEED, FIRST, count_of('n64'), sources_of('n64'), T)
    with engine(monkeypatch, 'n64', wide=True) as eng:
        assert eng.wide
        check(eng, 'n64')
        wide = eng.influence_sampled(SEED, FIRST, count_of('n64'), sources_of('n64'), T)
    assert np.array_equal(lane[0], wide[0]) and np.array_equal(lane[1], wide[1])


def test_disjoint_ranges_add_up(monkeypatch):
    name, cut = 'n300', 101
    count, sources = count_of(name), sources_of(name)
    want, want_merged = expect(name)
    with engine(monkeypatch, name) as eng:
        a = eng.influence_sampled(SEED, FIRST, cut, sources, T)
        b = eng.influence_sampled(SEED, FIRST + cut, count - cut, sources, T)
    assert np.array_equal(a[0].astype(np.int64) + b[0], want)
    assert np.array_equal(a[1].astype(np.int64) + b[1].astype(np.int64), want_merged)
    head = influence_cases.counts(name, count=cut)
    assert np.array_equal(a[0], head[0]) and np.array_equal(a[1], head[1])


def test_a_subset_and_a_reversed_list_give_the_same_rows(monkeypatch):
    name = 'n1024'
    count, sources = count_of(name), list(sources_of(name))
    want, want_merged = expect(name)
    with engine(monkeypatch, name) as eng:
        picked = [sources[i] for i in (5, 0, 11)]
        got, merged, _ = eng.influence_sampled(SEED, FIRST, count, picked, T)
        assert np.array_equal(got, want[[5, 0, 11]]) and np.array_equal(merged, want_merged[[5, 0, 11]])
        got, merged, _ = eng.influence_sampled(SEED, FIRST, count, sources[::-1], T)
        assert np.array_equal(got, want[::-1]) and np.array_equal(merged, want_merged[::-1])


@pytest.mark.parametrize('name', ['n64', 'n1024'])
def test_a_chunk_below_a_group_gives_the_same_arrays(monkeypatch, name):
    """BSX_WIDE_CHUNK = 1 is clamped to one group per launch: n_sources * G_per launches, G_per = 2 for G + 37 samples."""
    assert count_of(name) == 32 * L_OF[name] + 37
    with engine(monkeypatch, name, chunk=1) as eng:
        stats = check(eng, name)
        assert stats['kernel_launches'] == 2 * len(sources_of(name))


def test_a_group_whose_pairs_have_all_merged_stops_stepping(monkeypatch):
    """Every rule of this network is a constant: all pairs merge at t = 1, and the merged counts behind it are filled in."""
    from test_gpu_wide_exact import yaml_of
    n, count, steps = 300, 32 * 16 + 37, 40
    text = yaml_of([[i] for i in range(n)], [0b11 if i % 2 else 0b00 for i in range(n)], ['any'] * n)
    sources = [0, 7, 299]
    with engine(monkeypatch) as eng:
        eng.set_problem(*problem_of(text))
        got, merged, stats = eng.influence_sampled(SEED, FIRST, count, sources, steps)
    assert not got.any()
    assert merged.tolist() == [[count] * steps] * len(sources)
    # items = n_sources * G_per, their valid counts sum to n_sources * count: one lock step (two updates per pair) each, at
    # most two
    assert stats['state_steps'] == 2 * len(sources) * count * steps
    assert 2 * len(sources) * count <= stats['executed_steps'] <= 4 * len(sources) * count


# ---- refusals: every check comes before a launch, and a failing call leaves the arrays alone ---------------------------

PATTERN32, PATTERN64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


def raw_call(eng, first, count, sources, steps, arrays='ism', n_sources=None, cells=1 << 12):
    """-> (status, error text, arrays untouched) of a direct call with pattern-filled arrays (those not in `arrays`: NULL).
    The arrays hold `cells` entries whatever the arguments say: a refused call must not write."""
    src = np.ascontiguousarray(sources, np.uint32)
    table = np.full(cells, PATTERN32, np.uint32)
    merged = np.full(cells, PATTERN64, np.uint64)
    rc = eng._lib.bsx_run_influence_sampled(eng._h, SEED, first, count, ptr(src) if 's' in arrays else None,
                                            len(src) if n_sources is None else n_sources, steps,
                                            ptr(table) if 'i' in arrays else None, ptr(merged) if 'm' in arrays else None,
                                            C.byref(_lib.Stats()))
    untouched = bool((table == np.uint32(PATTERN32)).all() and (merged == np.uint64(PATTERN64)).all())
    return rc, eng._lib.bsx_last_error(eng._h).decode(), untouched


def test_nothing_set_is_a_state_error(monkeypatch):
    with engine(monkeypatch) as eng:
        assert raw_call(eng, 0, 10, [0], T)[::2] == (ERR_STATE, True)


def test_argument_errors_on_n20(monkeypatch):
    """n20 has fixed-node variations and is refused for them; the checks of the arguments come first.  Its nodes 3 and 5
    are fixed (by variations: the origin leaves them free), so the origin-fixed refusal is tested on plain_n20 below."""
    net, space, _ = influence_cases.damage_cases.sampled_cases.compiled('n20')
    errors = [
        (dict(first=0, count=10, sources=[0], steps=T, arrays='sm'), ERR_INVALID, ['influence is null']),
        (dict(first=0, count=10, sources=[0], steps=T, arrays='im'), ERR_INVALID, ['sources is null']),
        (dict(first=0, count=10, sources=[0], steps=T, n_sources=0), ERR_INVALID, ['n_sources']),
        (dict(first=0, count=10, sources=[0], steps=0), ERR_INVALID, ['n_steps']),
        (dict(first=2 ** 64 - 5, count=10, sources=[0], steps=T), ERR_INVALID, ['wraps']),
        (dict(first=0, count=10, sources=[0, 20], steps=T), ERR_INVALID, ['sources[1]', 'node 20', 'not a node']),
        (dict(first=0, count=10, sources=[4, 0, 9, 0], steps=T), ERR_INVALID, ['sources[3]', 'node 0', 'twice']),
        (dict(first=0, count=2 ** 31 + 1, sources=[0], steps=T), ERR_RANGE_TOO_LARGE, ['2^31']),
        # 3355444 * 20 > 2^26 >= 3355443 * 20
        (dict(first=0, count=10, sources=[0], steps=3355444), ERR_UNSUPPORTED, ['BSX_INFLUENCE_MAX_CELLS']),
    ]
    with engine(monkeypatch) as eng:
        eng.set_problem(net, space)
        assert not eng.wide
        for kw, status, words in errors:
            rc, text, untouched = raw_call(eng, kw.pop('first'), kw.pop('count'), kw.pop('sources'), kw.pop('steps'), **kw)
            assert (rc, untouched) == (status, True) and all(w in text for w in words), (rc, text)
        for steps in (T, 3355443):
            rc, text, untouched = raw_call(eng, 0, 10, [0], steps)
            assert (rc, untouched) == (ERR_UNSUPPORTED, True) and 'fixed-node variations' in text, text


def plain_n20():
    """n20 of sampled_cases with its two fixed-node variations made plain fixed nodes: 18 free nodes."""
    from sampled_cases import any_case
    return problem_of(any_case(20, 2, 2020, range(0, 20, 2), fixed={3: '1', 5: '0'}))


def test_fixed_sources_and_an_empty_range(monkeypatch):
    net, space = plain_n20()
    n = net.n_nodes
    free = [i for i in range(n) if i not in (3, 5)]
    with engine(monkeypatch) as eng:
        eng.set_problem(net, space)
        rc, text, untouched = raw_call(eng, 0, 10, [0, 1, 5], T)
        assert (rc, untouched) == (ERR_INVALID, True) and all(w in text for w in ('sources[2]', 'node 5', 'fixed by the origin')), text
        # (a call that succeeds writes all its cells: arrays of the call's own size)
        rc, _, untouched = raw_call(eng, 0, 10, free, T, cells=len(free) * T * n)
        assert rc == 0 and not untouched
        # n_samples == 0: BSX_OK, zeros written, whatever the first sample is
        src = np.array(free, np.uint32)
        table = np.full(len(free) * T * n, 7, np.uint32)
        merged = np.full(len(free) * T, 7, np.uint64)
        assert eng._lib.bsx_run_influence_sampled(eng._h, SEED, 5, 0, ptr(src), len(src), T, ptr(table), ptr(merged), None) == 0
        assert not table.any() and not merged.any()


def test_the_cell_limit_and_the_product_limit_at_1024_nodes(monkeypatch):
    """16 sources * 4096 steps * 1024 nodes = 2^26 cells are admitted, one step more is not; so are 2^40 trajectories, and
    2^31 more are not.  Neither call gets arrays of
    that size: the space has a fixed-node variation, whose refusal comes behind the cell count, so the admitted size shows
    in the text of the refusal and nothing is written either way."""
    from sampled_cases import any_case
    sources = list(range(16))
    assert 16 * 4096 * 1024 == _lib.INFLUENCE_MAX_CELLS
    with engine(monkeypatch) as eng:
        eng.set_problem(*problem_of(any_case(1024, 2, 3, range(0, 40), fixed={300: '0?'})))
        assert eng.wide
        rc, text, untouched = raw_call(eng, 0, 10, sources, 4097)
        assert (rc, untouched) == (ERR_UNSUPPORTED, True) and 'BSX_INFLUENCE_MAX_CELLS' in text, text
        rc, text, untouched = raw_call(eng, 0, 10, sources, 4096)
        assert (rc, untouched) == (ERR_UNSUPPORTED, True) and 'fixed-node variations' in text, text
        # n_sources * n_samples: 513 * 2^31 > 2^40 = 512 * 2^31, refused ahead of the cell count
        rc, text, untouched = raw_call(eng, 0, 2 ** 31, list(range(300)) + list(range(301, 514)), 2 ** 20)
        assert (rc, untouched) == (ERR_RANGE_TOO_LARGE, True) and '2^40' in text, text


@pytest.mark.parametrize('name,word', [('n700_variations', 'fixed-node variations'), ('n600_9_inputs', 'fixed-node variations')])
def test_spaces_with_variations_are_refused(monkeypatch, name, word):
    net, space, _ = influence_cases.damage_cases.sampled_cases.compiled(name)
    with engine(monkeypatch) as eng:
        eng.set_problem(net, space)
        rc, text, untouched = raw_call(eng, 0, 10, [0], T)
        assert (rc, untouched) == (ERR_UNSUPPORTED, True) and word in text, text


def test_a_schedule_and_perturbation_variations_are_refused(monkeypatch):
    from sampled_cases import any_case
    for perturbations, word in (({10: {'1': '2'}}, 'schedule'), ({10: {'0?': '3'}}, 'perturbation variations')):
        text = any_case(300, 2, 2, range(0, 40), perturbations=perturbations)
        with engine(monkeypatch) as eng:
            eng.set_problem(*problem_of(text))
            rc, err, untouched = raw_call(eng, 0, 10, [0], T)
            assert (rc, untouched) == (ERR_UNSUPPORTED, True) and word in err, err
