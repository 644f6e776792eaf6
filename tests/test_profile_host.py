"""
Host side of the attractor profile, checked without a GPU:

* the vertical counters of the profile kernels (boolsi_amd/csrc/bsx_planes.h).  tests/profile_check.cpp is a
  stand-alone program that the host C++ compiler builds with no HIP include path, so it compiles exactly the functions
  the kernels call; it is built a second time with the address and undefined-behaviour sanitizers and run as its own
  process;
* find_node_correlations on attractors that carry only `activity` (on-counts / length, what the device returns)
  against the same attractors carrying only `states`: the arrays must be equal, not close.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from boolsi_amd.attract import AggregatedAttractor
from boolsi_amd.attractor_analysis import find_node_correlations
from boolsi_amd.model import decode_state

from util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_profile_check(tmp_path, extra):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'profile_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror'] + extra +
                          ['-I' + os.path.join(ROOT, 'boolsi_amd', 'csrc'), os.path.join(ROOT, 'tests', 'profile_check.cpp'), '-o', exe])
    return exe


@pytest.mark.parametrize('flags', [[], ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']],
                         ids=['plain', 'sanitized'])
def test_planes_count_like_integers(tmp_path, flags):
    exe = build_profile_check(tmp_path, flags)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    word, compared = res.stdout.split()
    assert word == 'ok' and int(compared) > 1_000_000       # (NW = 1, 2, 4, 8; six run lengths; three widths and densities)


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def attractor_sets():
    """(name, [(key, length, frequency, states as lists of bool)]) from the golden attract examples and a hand-made set"""
    sets = []
    for case in load('attract_examples.json'):
        rows = (case.get('master') or {}).get('rows')
        if not rows or 'states' not in rows[0]:
            continue
        n = len(case['cfg']['node_names'])
        sets.append((case['name'], [(int(r['key']), r['length'], r['frequency'], [decode_state(int(c), n) for c in r['states']])
                                    for r in rows]))
    # a 3-cycle, a 2-cycle and fixed points over five nodes, unequal frequencies (lengths that do not divide evenly)
    b = lambda text: [ch == '1' for ch in text]
    sets.append(('hand', [
        (1, 3, 7, [b('10000'), b('01010'), b('11010')]),
        (2, 2, 5, [b('01001'), b('00111')]),
        (3, 1, 11, [b('11100')]),
        (4, 1, 2, [b('00011')]),
        (5, 3, 1, [b('00001'), b('10001'), b('10101')]),
    ]))
    return sets


def test_sets_are_not_vacuous():
    sets = attractor_sets()
    assert len(sets) >= 2 and sets[-1][0] == 'hand'
    assert any(len(rows) >= 2 for name, rows in sets if name != 'hand')
    assert any(length == 3 for _, length, _, _ in sets[-1][1])
    assert len({f for _, _, f, _ in sets[-1][1]}) > 1


@pytest.mark.parametrize('name', [name for name, _ in attractor_sets()])
def test_correlations_from_activity_equal_those_from_states(name):
    rows = dict(attractor_sets())[name]
    with_states = [AggregatedAttractor(key, length, f, 0, 0, states) for key, length, f, states in rows]
    with_activity = []
    for key, length, f, states in rows:
        on_counts = np.array(states, dtype=np.uint32).sum(axis=0, dtype=np.uint32)      # what the device counts
        with_activity.append(AggregatedAttractor(key, length, f, 0, 0, None, activity=on_counts.astype(np.float64) / length))
        assert with_activity[-1].states is None
        assert np.array_equal(with_activity[-1].activity, np.mean(np.array(states, dtype=float), axis=0))
    a, b = find_node_correlations(with_states), find_node_correlations(with_activity)
    if a is None:
        assert b is None and (len(rows) == 1 or sum(f for _, _, f, _ in rows) <= 2)
        return
    assert same(a[0], b[0]) and same(a[1], b[1])
