"""
Target over sampled initial conditions (bsx_run_target_sampled) against the exact reference: sample_ref.sample_indices
turns sample numbers into flat problem indices, WideRef's search runs them (sampled_target_cases.py).  Every comparison
is exact equality on integers: the count, the histogram, the hit lists, stats.problems and state_steps.

A range is 32 L + 37 samples from FIRST with SEED: unaligned, with a ragged second group.  The substates are hit at
several times, later than every T_p, in both groups, and missed by samples whose cycle closes first: at max_t = inf every
miss is a closed cycle.
"""
import ctypes as C

import numpy as np
import pytest

from boolsi_amd import _lib
from boolsi_amd.compile import code_to_words

from sampled_cases import FIRST, L_OF, SEED, compiled
from sampled_target_cases import GENEROUS, INF, TARGETS, count_of, expect_target, histogram, hits_of, target_ends
from test_gpu_sampled import ERR_INVALID, ERR_STATE, ERR_STEP_LIMIT, engine

pytestmark = pytest.mark.gpu


def words(name):
    net = compiled(name)[0]
    nodes, code, _ = TARGETS[name]
    return code_to_words(sum(1 << i for i in nodes), net.n_words), code_to_words(code, net.n_words)


def pairs(hits):
    return [(int(h['offset']), int(h['t'])) for h in hits]


def check(eng, name, first, count, max_t, want_hits, want_steps=None):
    """check_target's shape (test_gpu_wide_exact.py) for a sampled call: count, 8-bin histogram, the whole list with
    cap = count, the first five with cap = 5, the statistics."""
    mask, code = words(name)
    n_hits, hist, listed, st = eng.target_sampled(SEED, first, count, max_t, mask, code, hist_bins=8, cap=count)
    assert n_hits == len(want_hits)
    assert hist.tolist() == histogram(want_hits)
    assert pairs(listed) == want_hits
    assert st['problems'] == count
    if want_steps is not None:
        assert st['state_steps'] == want_steps
    n5, hist5, first5, st5 = eng.target_sampled(SEED, first, count, max_t, mask, code, hist_bins=8, cap=5)
    assert n5 == n_hits and hist5.tolist() == hist.tolist() and pairs(first5) == want_hits[:5]
    assert st5['state_steps'] == st['state_steps']
    return n_hits, hist.tolist(), pairs(listed), st


# ---- the wide family -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['n257', 'n577', 'n600_9_inputs', 'n1024', 'n700_variations'])
def test_target_sampled_at_a_splitting_a_generous_cap_and_without_one(monkeypatch, name):
    want = expect_target(name)
    with engine(monkeypatch, name) as eng:
        assert eng.wide
        for cap in (TARGETS[name][2], GENEROUS, INF):
            hits, steps = want[cap]
            check(eng, name, FIRST, count_of(name), cap, hits, steps)


# ---- handles of the <= 256-node family: the second lowering ----------------------------------------------------------

@pytest.mark.parametrize('name', ['n64', 'example2'])
def test_per_lane_handle_and_wide_handle_agree(monkeypatch, name):
    want = expect_target(name)
    net, space, _ = compiled(name)
    mask, code = words(name)
    n_enum = min(space.n_problems, 4096)
    caps = (TARGETS[name][2], GENEROUS, INF)
    with engine(monkeypatch, name) as eng:
        assert not eng.wide
        before = eng.target(0, n_enum, GENEROUS, mask, code)[0].copy()
        lane = [check(eng, name, FIRST, count_of(name), cap, *want[cap])[:3] for cap in caps]
        after = eng.target(0, n_enum, GENEROUS, mask, code)[0]
        assert len(before) and pairs(after) == pairs(before)
        # a new space drops the second lowering: the next sampled call lowers again and gives the same
        eng.set_space(space)
        assert check(eng, name, FIRST, count_of(name), INF, *want[INF])[:3] == lane[2]
    with engine(monkeypatch, name, wide=True) as eng:
        assert eng.wide
        wide = [check(eng, name, FIRST, count_of(name), cap, *want[cap])[:3] for cap in caps]
    assert lane == wide


# ---- ranges, launches, the host-reduce path --------------------------------------------------------------------------

RANGES = 'n577'


def test_three_launches_three_calls_one_wait_and_the_host_path(monkeypatch):
    G = 32 * L_OF[RANGES]
    count = 2 * G + 37                      # three launches of at most G samples
    ends = target_ends(RANGES, FIRST, count, INF)
    want, steps = hits_of(ends), sum(t for _, t in ends)
    assert any(q >= 2 * G for q, _ in want) and 0 < len(want) < count
    cuts = [0, 100, G + 5, count]           # three ragged calls, none of them whole groups
    mask, code = words(RANGES)
    with engine(monkeypatch, RANGES, chunk=G) as eng:
        n_hits, hist, listed, st = check(eng, RANGES, FIRST, count, INF, want, steps)
        assert st['kernel_launches'] == 6        # three launches, each with its reduction right behind it
        parts = [eng.target_sampled(SEED, FIRST + a, b - a, INF, mask, code, hist_bins=8, cap=b - a) for a, b in zip(cuts, cuts[1:])]
        assert sum(p[0] for p in parts) == n_hits
        assert np.sum([p[1] for p in parts], axis=0).tolist() == hist
        assert [(a + q, t) for (a, _), p in zip(zip(cuts, cuts[1:]), parts) for q, t in pairs(p[2])] == listed
        # (T_p = 0 for every sample of this case, so a search ends at the same time whatever group it is in)
        assert sum(p[3]['state_steps'] for p in parts) == steps
        # cap = 0: nothing is listed, and the host waits once: one run of launches between the timing events
        n0, hist0, none, st0 = eng.target_sampled(SEED, FIRST, count, INF, mask, code, hist_bins=8, cap=0)
        assert n0 == n_hits and hist0.tolist() == hist and len(none) == 0
        assert st0['kernel_launches'] == 6 and st0['state_steps'] == steps
        bare = eng.target_sampled(SEED, FIRST, count, INF, mask, code)       # no histogram either
        assert bare[0] == n_hits and len(bare[1]) == 0 and len(bare[2]) == 0
        empty = eng.target_sampled(SEED, FIRST, 0, INF, mask, code, hist_bins=8, cap=4)
        assert empty[0] == 0 and empty[1].tolist() == [0] * 8 and len(empty[2]) == 0 and empty[3]['problems'] == 0
    with engine(monkeypatch, RANGES, chunk=G, host=True) as eng:
        host = check(eng, RANGES, FIRST, count, INF, want, steps)
        assert host[:3] == (n_hits, hist, listed)
        n0, hist0, none, _ = eng.target_sampled(SEED, FIRST, count, INF, mask, code, hist_bins=8, cap=0)
        assert n0 == n_hits and hist0.tolist() == hist and len(none) == 0


# ---- refusals --------------------------------------------------------------------------------------------------------

def raw_call(eng, first, count, max_t, mask, code, hist, hits):
    n_hits, n_listed, st = C.c_uint64(), C.c_uint64(), _lib.Stats()
    return eng._lib.bsx_run_target_sampled(eng._h, SEED, first, count, max_t, _lib.ptr(mask), _lib.ptr(code), _lib.ptr(hist), len(hist),
                                           _lib.ptr(hits), len(hits), C.byref(n_hits), C.byref(n_listed), C.byref(st))


def test_refusals(monkeypatch):
    name = 'n577'
    mask, code = words(name)
    with engine(monkeypatch, name) as eng:
        with pytest.raises(_lib.EngineError) as e:
            eng.target_sampled(SEED, 2 ** 64 - 10, 10, GENEROUS, mask, code, hist_bins=8, cap=10)     # first + n = 2^64 wraps to 0
        assert e.value.status == ERR_INVALID
        ends = target_ends(name, 2 ** 64 - 11, 10, GENEROUS)          # ... the last range that does not
        check(eng, name, 2 ** 64 - 11, 10, GENEROUS, hits_of(ends), sum(t for _, t in ends))
        with pytest.raises(_lib.EngineError) as e:
            eng.target_sampled(SEED, 0, 10, GENEROUS, mask, code, hist_bins=2049)
        assert e.value.status == ERR_INVALID
    with engine(monkeypatch) as eng:
        hist, hits = np.zeros(8, np.uint64), np.zeros(4, _lib.HIT)
        assert raw_call(eng, 0, 10, 100, mask, code, hist, hits) == ERR_STATE


def test_step_limit_on_a_chaotic_network(monkeypatch):
    """Unbiased K = 3 tables at n = 300 do not close a cycle within 512 steps, and the all-ones substate of five nodes is
    not reached by then: with max_t = inf that is the step limit, and nothing is written."""
    from boolsi_amd import synth
    from boolsi_amd.compile import compile_problem
    from boolsi_amd.constants import Mode
    from boolsi_amd.engine import Engine
    from boolsi_amd.input import parse_input_text
    import sample_ref
    from test_gpu_wide_exact import yaml_of
    from wide_ref import WideRef
    preds, masks = synth.random_network(300, 3, 77)
    net, space = compile_problem(parse_input_text(yaml_of(preds, masks, ['any'] * 300), 100000, Mode.SIMULATE))
    idx = sample_ref.sample_indices(space, SEED, range(8))
    nodes = list(range(100, 130))
    all_ones = sum(1 << i for i in nodes)
    res = WideRef(net, space).target(idx, 600, nodes, all_ones)
    assert not any(reached for reached, _ in res) and all(t == 600 for _, t in res)     # no hit, no closed cycle by t = 600
    mask, code = code_to_words(all_ones, net.n_words), code_to_words(all_ones, net.n_words)
    with monkeypatch.context() as mp:
        mp.setenv('BSX_WIDE_STEP_LIMIT', '512')
        eng = Engine(0)
        try:
            eng.set_problem(net, space)
            sentinel = np.full(8, 0xAB, np.uint8).view(np.uint64)[0]
            hist = np.full(8, sentinel, np.uint64)
            hits = np.zeros(8, _lib.HIT)
            hits['offset'] = hits['t'] = sentinel
            assert raw_call(eng, 0, 8, _lib.T_INF, mask, code, hist, hits) == ERR_STEP_LIMIT
            assert (hist == sentinel).all() and (hits['offset'] == sentinel).all() and (hits['t'] == sentinel).all()
        finally:
            eng.close()
