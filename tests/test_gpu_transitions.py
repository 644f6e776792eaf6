"""
bsx_run_attractor_transitions / Engine.attractor_transitions: where every single-node flip of every cycle state of a
listed attractor table ends, in one device call.  Every comparison is exact equality.

Reference: tests/trans_ref.py (dict-based, the CPU oracle's step; pinned to the oracle's attract by
tests/test_trans_ref.py).  Each case first asserts from the reference alone that it is not vacuous.  The two cases
that need their own environment (a lowered BSX_TRANS_STEP_LIMIT, BSX_WIDE=1) run in a fresh child process: this file,
with the case's name as its argument.
"""
import csv
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == '__main__':
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from boolsi_amd import _lib
from boolsi_amd.attract import run_attract_range
from boolsi_amd.engine import Engine, EngineError

import trans_ref
from test_gpu_profile import (WIDTH_CASES, compiled, lfsr_cycle_length, lfsr_text, mixed_attractors, oracle_table,
                              random_text)

pytestmark = pytest.mark.gpu
INF = float('inf')
OUTSIDE, UNRESOLVED = trans_ref.OUTSIDE, trans_ref.UNRESOLVED
assert (OUTSIDE, UNRESOLVED) == (_lib.TRANS_OUTSIDE, _lib.TRANS_UNRESOLVED)
EXAMPLE2_DIR = os.path.join(ROOT, 'tests', 'golden', 'examples', 'output3_example2')


def tuples(edges):
    assert edges.dtype == _lib.TRANS_EDGE and _lib.TRANS_EDGE.itemsize == 24
    return [(int(e['src']), int(e['dst']), int(e['count']), int(e['sum_mu'])) for e in edges]


def check_call(eng, ref, max_t=INF, want=None):
    """one call against the reference: edges, node_exits, closed, the row sums and the statistics -> the reference's result"""
    want = want or ref.transitions(max_t)
    edges_want, exits_want, _ = want
    edges, exits, closed = eng.attractor_transitions(ref.keys, ref.lengths, max_t=max_t, node_exits=True)
    got = tuples(edges)
    assert got == edges_want
    assert exits.dtype == np.uint32 and np.array_equal(exits, exits_want)
    assert closed.tolist() == [1] * len(ref.keys)
    for q, length in enumerate(ref.lengths):
        assert sum(e[2] for e in got if e[0] == q) == length * len(ref.free)
    st = eng.trans_stats
    assert st['problems'] == sum(ref.lengths) * len(ref.free) and st['state_steps'] == sum(e[3] for e in got)
    assert st['kernel_launches'] == 4 and st['executed_steps'] >= sum(ref.lengths) + st['state_steps']
    edges2, none, _ = eng.attractor_transitions(ref.keys, ref.lengths, max_t=max_t)
    assert none is None and tuples(edges2) == got
    return want


@functools.lru_cache(maxsize=None)
def width_ref(name):
    n, seed, fixed, many = WIDTH_CASES[name]
    _, net, space = compiled(random_text(n, seed, fixed=fixed, many_preds=many))
    table = oracle_table(net, space, 1 << 10)
    keys = sorted(table)
    return trans_ref.TransRef(net, space, keys, [table[k] for k in keys])


@functools.lru_cache(maxsize=None)
def example2_ref():
    _, net, space = compiled(open(os.path.join(EXAMPLE2_DIR, 'example2.yaml')).read())
    table = oracle_table(net, space, 8)
    keys = sorted(table, key=lambda k: -table[k])          # (the CLI's order: the 3-cycle first)
    return trans_ref.TransRef(net, space, keys, [table[k] for k in keys])


@pytest.fixture(scope='module')
def eng():
    with Engine(0) as e:
        yield e


# ---- the smallest case --------------------------------------------------------------------------------------------------

def test_example2(eng):
    ref = example2_ref()
    edges, _, _ = ref.transitions()
    assert ref.lengths == [3, 1] and sum(e[2] for e in edges) == 12 and len(edges) == 3 and len(trans_ref.cross_edges(edges)) == 2
    eng.set_problem(ref.net, ref.space)
    check_call(eng, ref)


def run_cli(args, out_dir):
    res = subprocess.run([sys.executable, '-m', 'boolsi_amd'] + args + ['-o', out_dir], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    return res.stdout


def test_cli_transitions_example2(tmp_path):
    ref = example2_ref()
    edges, _, _ = ref.transitions()
    yaml = os.path.join(EXAMPLE2_DIR, 'example2.yaml')
    run_cli(['attract', yaml], str(tmp_path / 'plain'))
    run_cli(['attract', yaml, '--transitions'], str(tmp_path / 'with'))
    plain = sorted(f for f in os.listdir(tmp_path / 'plain') if f.endswith('.csv'))
    assert plain == ['attractor_summaries.csv', 'attractors.csv', 'node_correlations.csv']
    assert sorted(f for f in os.listdir(tmp_path / 'with') if f.endswith('.csv')) == sorted(plain + ['attractor_transitions.csv'])
    for name in plain:
        assert open(tmp_path / 'plain' / name, 'rb').read() == open(tmp_path / 'with' / name, 'rb').read(), name
    summaries = list(csv.reader(open(tmp_path / 'with' / 'attractor_summaries.csv')))[1:]
    ids = [r[0] for r in summaries]
    assert [int(r[1]) for r in summaries] == ref.lengths            # guard: the reference's rows are in the CLI's order
    text = open(tmp_path / 'with' / 'attractor_transitions.csv', newline='').read()
    header = 'attractor_id,destination_id,n_perturbations,share,recovery_time_mean'
    assert text == '\r\n'.join([header] + trans_ref.csv_rows(edges, ids, ref.lengths, 3)) + '\r\n'
    # a cap: the run's -t is the call's max_t
    run_cli(['attract', yaml, '--transitions', '-t', '4'], str(tmp_path / 'capped'))
    capped, _, detail = ref.transitions(4)
    assert detail['unresolved'] > 0 and capped != edges                 # guard
    summaries = [r for r in csv.reader(open(tmp_path / 'capped' / 'attractor_summaries.csv')) if r[0].startswith('attractor') and r[0] != 'attractor_id']
    assert [r[0] for r in summaries] == ids and [int(r[1]) for r in summaries] == ref.lengths      # guard: both are found within 4 steps
    text = open(tmp_path / 'capped' / 'attractor_transitions.csv', newline='').read()
    assert text == '\r\n'.join([header] + trans_ref.csv_rows(capped, ids, ref.lengths, 3)) + '\r\n'


# ---- every state width, fixed nodes, a node beyond the mux tree -----------------------------------------------------------

@pytest.mark.parametrize('name', list(WIDTH_CASES))
def test_width(eng, name):
    ref = width_ref(name)
    want = ref.transitions()
    edges, exits, detail = want
    assert len(trans_ref.cross_edges(edges)) >= 2 and detail['unresolved'] == 0        # guards
    if name in ('n100', 'n256', 'n100_many_preds'):
        assert detail['outside'] > 0
    if name == 'n64_fixed':
        assert len(ref.free) == 62 and not exits[:, [20, 41]].any() and exits.any()
    eng.set_problem(ref.net, ref.space)
    check_call(eng, ref, want=want)


@pytest.mark.parametrize('max_t', [INF, 19, 18, 5, 0])
def test_caps_n64(eng, max_t):
    ref = width_ref('n64')
    want = ref.transitions(max_t)
    flips, unresolved = sum(ref.lengths) * 64, want[2]['unresolved']
    assert {INF: unresolved == 0, 19: unresolved == 0, 18: 0 < unresolved, 5: 0 < unresolved < flips, 0: unresolved == flips}[max_t]
    if max_t == 18:
        assert ref.transitions(19)[2]['max_mu'] == 15 and ref.lengths == [4, 4]
    eng.set_problem(ref.net, ref.space)
    check_call(eng, ref, max_t, want)


def test_cap_splits_unlisted_cycles_n100(eng):
    ref = width_ref('n100')
    want = ref.transitions(14)
    detail = want[2]
    assert detail['outside'] > 0 and detail['outside_total'] - detail['outside'] > 0        # guard: both sides of the cap
    eng.set_problem(ref.net, ref.space)
    check_call(eng, ref, 14, want)


# ---- many workgroups, divergent rows, more edges than a workgroup's LDS table holds -----------------------------------------

@functools.lru_cache(maxsize=None)
def mixed_ref(rows):
    net, space, keys, lengths = mixed_attractors()
    ref = trans_ref.TransRef(net, space, keys[:rows], lengths[:rows])
    return ref, ref.transitions()


def test_mixed(eng):
    ref, want = mixed_ref(128)
    edges, _, detail = want
    assert sum(ref.lengths) == 65536 and sum(e[2] for e in edges) == 1 << 20
    assert len(edges) == 960 and len(trans_ref.cross_edges(edges)) == 896 and all(e[3] == 0 for e in edges)
    eng.set_problem(ref.net, ref.space)
    check_call(eng, ref, want=want)
    got, _, _ = eng.attractor_transitions(ref.keys, ref.lengths, edge_cap=960)
    assert tuples(got) == edges
    with pytest.raises(EngineError) as err:
        eng.attractor_transitions(ref.keys, ref.lengths, edge_cap=959)
    assert err.value.status == _lib.ERR_TABLE_FULL


def test_mixed_half_table(eng):
    ref, want = mixed_ref(64)
    full = mixed_ref(128)[1][0]
    assert want[2]['outside'] == sum(e[2] for e in full if e[0] < 64 and 64 <= e[1] < OUTSIDE) > 0      # guard
    eng.set_problem(ref.net, ref.space)
    check_call(eng, ref, want=want)


# ---- long cycles, listed and unlisted -----------------------------------------------------------------------------------

def test_unlisted_long_cycle(eng):
    assert lfsr_cycle_length(10, 7) == 1023
    _, net, space = compiled(lfsr_text(10, 7))
    ref = trans_ref.TransRef(net, space, [0], [1])
    eng.set_problem(net, space)
    for max_t, dst in ((INF, OUTSIDE), (1023, OUTSIDE), (1022, UNRESOLVED)):
        want = ref.transitions(max_t)
        assert want[0] == [(0, dst, 10, 0)]
        check_call(eng, ref, max_t, want)


def child(case):
    res = subprocess.run([sys.executable, os.path.abspath(__file__), case], capture_output=True, text=True, timeout=60,
                         env=dict(os.environ, **CHILD_ENV[case]))
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    assert res.stdout.strip().endswith(case + ' ok')


CHILD_ENV = {'step_limit': {'BSX_TRANS_STEP_LIMIT': '512'}, 'wide': {'BSX_WIDE': '1'}}


def child_step_limit():
    _, net, space = compiled(lfsr_text(10, 7))
    with Engine(0) as e:
        e.set_problem(net, space)
        edges, _, _ = e.attractor_transitions([0], [1], max_t=100)          # decided well below the limit
        assert tuples(edges) == [(0, UNRESOLVED, 10, 0)]
        try:
            e.attractor_transitions([0], [1])
        except EngineError as err:
            assert err.status == _lib.ERR_STEP_LIMIT, err
        else:
            raise AssertionError('no error')


def child_wide():
    ref = example2_ref()
    with Engine(0) as e:
        e.set_problem(ref.net, ref.space)
        assert e.wide
        try:
            e.attractor_transitions(ref.keys, ref.lengths)
        except EngineError as err:
            assert err.status == _lib.ERR_UNSUPPORTED and 'wide' in str(err), err
        else:
            raise AssertionError('no error')


def test_step_limit_in_a_child():
    child('step_limit')


def test_wide_family_is_refused_in_a_child():
    child('wide')


def test_listed_long_cycle(eng):
    n, lam = 17, (1 << 17) - 1
    assert lfsr_cycle_length(n, 14) == lam
    _, net, space = compiled(lfsr_text(n, 14))
    eng.set_problem(net, space)
    edges, exits, closed = eng.attractor_transitions([1, 0], [lam, 1], node_exits=True)
    # every non-zero state is on the cycle: a flip of a cycle state leaves it only from the n states with one node on, by
    # that node, into the fixed point 0; every flip of 0 lands on the cycle; mu = 0 throughout
    assert tuples(edges) == [(0, 0, n * lam - n, 0), (0, 1, n, 0), (1, 0, n, 0)]
    assert exits.tolist() == [[1] * n, [1] * n] and closed.tolist() == [1, 1]
    assert eng.trans_stats['problems'] == n * (lam + 1) and eng.trans_stats['state_steps'] == 0


# ---- refusals and hygiene -----------------------------------------------------------------------------------------------

def test_refusals(eng):
    net, space, keys, lengths = mixed_attractors()
    eng.set_problem(net, space)
    q = lengths.index(1023)
    fixed_point = keys[lengths.index(1)]
    for bad_keys, bad_lengths, row in (([fixed_point, keys[q]], [1, 1022], 1),                  # a length one short: not closed
                                       ([keys[q], fixed_point, keys[q]], [1023, 1, 1023], 2),   # a duplicated row
                                       ([keys[q], fixed_point], [1023, 2], 1)):                 # a multiple of the period
        with pytest.raises(EngineError) as err:
            eng.attractor_transitions(bad_keys, bad_lengths, node_exits=True)
        assert err.value.status == _lib.ERR_INVALID and 'row {} '.format(row) in str(err.value), str(err.value)
    with pytest.raises(EngineError) as err:
        eng.attractor_transitions([keys[q]], [0])
    assert err.value.status == _lib.ERR_INVALID
    edges, exits, closed = eng.attractor_transitions([], [], node_exits=True)
    assert len(edges) == 0 and exits.shape == (0, 16) and len(closed) == 0
    assert eng.trans_stats['problems'] == 0 and eng.trans_stats['kernel_launches'] == 0


def test_handle_state_is_left_alone(eng):
    ref = width_ref('n64')
    eng.set_problem(ref.net, ref.space)
    run_attract_range(eng, 0, 1 << 10)                                  # (fills the cycle journal)
    before, none_before, stats_before = run_attract_range(eng, 0, 1 << 10)
    eng.attractor_transitions(ref.keys, ref.lengths, node_exits=True)
    after, none_after, stats_after = run_attract_range(eng, 0, 1 << 10)
    assert {k: e[0] for k, e in before.items()} == dict(zip(ref.keys, ref.lengths))
    assert after == before and none_after == none_before
    assert stats_after['executed_steps'] == stats_before['executed_steps'] and stats_after['state_steps'] == stats_before['state_steps']


if __name__ == '__main__':
    {'step_limit': child_step_limit, 'wide': child_wide}[sys.argv[1]]()
    print(sys.argv[1] + ' ok')
