"""
Damage spreading over sampled pairs of states (bsx_run_damage_sampled) against the exact reference: damage_ref restates
the definition of include/bsx.h in Python ints over sample_ref and WideRef.rules.  Every comparison is exact equality on
integers: the three sums and the whole histogram, for every t.

damage_cases.expect builds the expected arrays from the reference alone and asserts, from the reference alone, that a
case is not vacuous.  A range is G + 37 samples from 1000003 (G = 32 L, a group): unaligned, with a ragged second group.
"""
import contextlib
import ctypes as C
import faulthandler

import numpy as np
import pytest

from boolsi_amd import _lib
from boolsi_amd._lib import ptr

import damage_cases
from damage_cases import CASES, FIRST, FLIPS, SEED, T, compiled, count_of, expect

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


def check(eng, name, h, first=FIRST, count=None, want=None):
    count = count_of(name) if count is None else count
    sum_d, sum_d2, merged, hist = want if want is not None else expect(name, h)
    got_d, got_d2, got_m, got_h, stats = eng.damage_sampled(SEED, first, count, h, T, hist=True)
    assert got_d.tolist() == sum_d
    assert got_d2.tolist() == sum_d2
    assert got_m.tolist() == merged
    assert got_h.tolist() == hist
    # the histogram carries the sums
    k = np.arange(got_h.shape[1], dtype=np.uint64)
    assert got_h.sum(axis=1).tolist() == [count] * (T + 1)
    assert (got_h * k).sum(axis=1).tolist() == sum_d and (got_h * k * k).sum(axis=1).tolist() == sum_d2
    assert got_h[:, 0].tolist() == merged
    assert stats['problems'] == count and stats['state_steps'] == 2 * count * T
    assert 0 < stats['executed_steps'] <= 2 * count * T
    # without the histogram: the same sums
    plain = eng.damage_sampled(SEED, first, count, h, T)
    assert plain[3] is None and [a.tolist() for a in plain[:3]] == [sum_d, sum_d2, merged]
    return stats


@pytest.mark.parametrize('h', FLIPS)
@pytest.mark.parametrize('name', list(CASES))
def test_damage_equals_the_reference(monkeypatch, name, h):
    net = compiled(name)[0]
    if name == 'n600_wide_inputs':
        assert sorted(len(p) for p in net.predecessor_lists)[-2:] == [9, 12]
    with engine(monkeypatch, name) as eng:
        assert eng.wide == (net.n_nodes > 256)
        check(eng, name, h)


def test_64_flips_at_1024_nodes(monkeypatch):
    with engine(monkeypatch, 'n1024') as eng:
        check(eng, 'n1024', 64)


@pytest.mark.parametrize('h', FLIPS)
def test_per_lane_handle_and_wide_handle_agree(monkeypatch, h):
    with engine(monkeypatch, 'n64', wide=True) as eng:
        assert eng.wide
        check(eng, 'n64', h)


def test_disjoint_ranges_add_up(monkeypatch):
    name, h = 'n300', 3
    count, cut = count_of(name), 101
    whole = expect(name, h)
    with engine(monkeypatch, name) as eng:
        a = eng.damage_sampled(SEED, FIRST, cut, h, T, hist=True)
        b = eng.damage_sampled(SEED, FIRST + cut, count - cut, h, T, hist=True)
    for x, y, want in zip(a[:4], b[:4], whole):
        assert (x + y).tolist() == want
    d = damage_cases.distances(name, h)
    assert a[0].tolist() == [int(row[:cut].sum()) for row in d]


@pytest.mark.parametrize('name', ['n64', 'n1024'])
def test_a_chunk_below_a_group_gives_the_same_arrays(monkeypatch, name):
    """BSX_WIDE_CHUNK = 1 is clamped to one group per launch: two launches for G + 37 samples."""
    with engine(monkeypatch, name, chunk=1) as eng:
        stats = check(eng, name, 3)
        assert stats['kernel_launches'] == 2


def test_a_group_whose_pairs_have_all_merged_stops_stepping(monkeypatch):
    """Every rule of this network is a constant: all pairs merge at t = 1, and the sums behind it are filled in."""
    from boolsi_amd.compile import compile_problem
    from boolsi_amd.constants import Mode
    from boolsi_amd.input import parse_input_text
    from test_gpu_wide_exact import yaml_of
    n, count, steps = 300, 32 * 16 + 37, 40
    text = yaml_of([[i] for i in range(n)], [0b11 if i % 2 else 0b00 for i in range(n)], ['any'] * n)
    net, space = compile_problem(parse_input_text(text, 100000, Mode.SIMULATE))
    with engine(monkeypatch) as eng:
        eng.set_problem(net, space)
        sum_d, sum_d2, merged, hist, stats = eng.damage_sampled(SEED, FIRST, count, 5, steps, hist=True)
    assert sum_d.tolist() == [5 * count] + [0] * steps and sum_d2.tolist() == [25 * count] + [0] * steps
    assert merged.tolist() == [0] + [count] * steps
    assert hist[0, 5] == count and hist[1:, 0].tolist() == [count] * steps and int(hist.sum()) == count * (steps + 1)
    assert stats['state_steps'] == 2 * count * steps and 2 * count <= stats['executed_steps'] <= 4 * count


def test_steps_beyond_the_lds_accumulators(monkeypatch):
    """More steps than a workgroup's LDS holds sums for (the groups then add to HBM), against fewer steps of the same
    samples, where the sums stay in LDS, and against the reference at t <= T."""
    name, h, steps = 'n1024', 3, 2000
    count = count_of(name)
    with engine(monkeypatch, name) as eng:
        long = eng.damage_sampled(SEED, FIRST, count, h, steps, hist=False)
        short = eng.damage_sampled(SEED, FIRST, count, h, 500, hist=False)
    want = expect(name, h)
    for q in range(3):
        assert long[q][:T + 1].tolist() == want[q]
        assert long[q][:501].tolist() == short[q].tolist()
    assert long[4]['state_steps'] == 2 * count * steps


# ---- refusals: every check comes before a launch, and a failing call leaves the arrays alone ---------------------------

PATTERN = 0xA5A5A5A5A5A5A5A5


def raw_call(eng, first, count, h, steps, arrays='dsmh', cells=1 << 16):
    """-> (status, error text, arrays untouched) of a direct call with pattern-filled arrays (those not in `arrays`: NULL).
    The arrays hold T + 1 entries (and `cells` histogram cells) whatever `steps` says: a refused call must not write."""
    bufs = {a: np.full(cells if a == 'h' else T + 1, PATTERN, np.uint64) for a in 'dsmh'}
    rc = eng._lib.bsx_run_damage_sampled(eng._h, SEED, first, count, h, steps, *[ptr(bufs[a]) if a in arrays else None for a in 'dsmh'],
                                         C.byref(_lib.Stats()))
    untouched = all((b == np.uint64(PATTERN)).all() for b in bufs.values())
    return rc, eng._lib.bsx_last_error(eng._h).decode(), untouched


def plain_n20():
    """n20 of sampled_cases with its two fixed-node variations made plain fixed nodes: 18 free nodes."""
    from boolsi_amd.compile import compile_problem
    from boolsi_amd.constants import Mode
    from boolsi_amd.input import parse_input_text
    from sampled_cases import any_case
    return compile_problem(parse_input_text(any_case(20, 2, 2020, range(0, 20, 2), fixed={3: '1', 5: '0'}), 100000, Mode.SIMULATE))


ARGUMENT_ERRORS = [
    ((2 ** 64 - 5, 10, 1, T), ERR_INVALID, 'wraps'),
    ((0, 10, 0, T), ERR_INVALID, 'n_flips'),
    ((0, 10, 65, T), ERR_INVALID, 'n_flips'),
    ((0, 2 ** 40 + 1, 1, T), ERR_RANGE_TOO_LARGE, '2^40'),
    ((0, 10, 1, 65536), ERR_UNSUPPORTED, '65535'),
]


def test_nothing_set_is_a_state_error(monkeypatch):
    with engine(monkeypatch) as eng:
        assert raw_call(eng, 0, 10, 1, T)[::2] == (ERR_STATE, True)


def test_argument_errors_on_n20(monkeypatch):
    """n20 has fixed-node variations and is refused for them; the checks of the arguments come first."""
    net, space, _ = damage_cases.sampled_cases.compiled('n20')
    with engine(monkeypatch) as eng:
        eng.set_problem(net, space)
        assert not eng.wide
        for args, status, word in ARGUMENT_ERRORS:
            rc, text, untouched = raw_call(eng, *args)
            assert (rc, untouched) == (status, True) and word in text, (args, rc, text)
        for present in ('smh', 'dmh', 'dsh'):
            rc, text, untouched = raw_call(eng, 0, 10, 1, T, arrays=present)
            assert (rc, untouched) == (ERR_INVALID, True) and 'null' in text
        rc, text, untouched = raw_call(eng, 0, 10, 1, T)
        assert (rc, untouched) == (ERR_UNSUPPORTED, True) and 'fixed-node variations' in text, text


def test_flips_beyond_the_free_nodes_and_an_empty_range(monkeypatch):
    net, space = plain_n20()
    n, n_free = net.n_nodes, net.n_nodes - len(space.fixed)
    assert (n, n_free) == (20, 18)
    with engine(monkeypatch) as eng:
        eng.set_problem(net, space)
        rc, text, untouched = raw_call(eng, 0, 10, n_free + 1, T)
        assert (rc, untouched) == (ERR_INVALID, True) and 'does not fix' in text
        rc, _, untouched = raw_call(eng, 0, 10, n_free, T)
        assert rc == 0 and not untouched
        sum_d, _, _, hist, _ = eng.damage_sampled(SEED, 0, 10, n_free, T, hist=True)
        assert sum_d[0] == 10 * n_free and hist[0, n_free] == 10
        # n_samples == 0: BSX_OK, zeros written
        d, s, m = (np.full(T + 1, 7, np.uint64) for _ in range(3))
        cells = np.full((T + 1) * (n + 1), 7, np.uint64)
        assert eng._lib.bsx_run_damage_sampled(eng._h, SEED, 5, 0, 1, T, ptr(d), ptr(s), ptr(m), ptr(cells), None) == 0
        assert not d.any() and not s.any() and not m.any() and not cells.any()


def test_a_histogram_of_more_than_2_to_24_cells(monkeypatch):
    """(16368 + 1) * 1025 > 2^24 at n = 1024; one step fewer fits."""
    assert 16369 * 1025 > 2 ** 24 >= 16368 * 1025
    with engine(monkeypatch, 'n1024') as eng:
        rc, text, untouched = raw_call(eng, 0, 10, 1, 16368)
        assert (rc, untouched) == (ERR_UNSUPPORTED, True) and '2^24' in text


@pytest.mark.parametrize('name,word', [('n700_variations', 'fixed-node variations'), ('n600_9_inputs', 'fixed-node variations')])
def test_spaces_with_variations_are_refused(monkeypatch, name, word):
    net, space, _ = damage_cases.sampled_cases.compiled(name)
    with engine(monkeypatch) as eng:
        eng.set_problem(net, space)
        rc, text, untouched = raw_call(eng, 0, 10, 1, T)
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
            rc, err, untouched = raw_call(eng, 0, 10, 1, T)
            assert (rc, untouched) == (ERR_UNSUPPORTED, True) and word in err, err
