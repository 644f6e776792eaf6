"""
Proof of tests/wide_ref.py (the numpy reference that pins the wide-state kernels above 256 nodes) against the CPU
oracle, at the sizes where both run: every field of the attract records, the table, the number of problems without
an attractor and the step count; simulate trajectories, finals and digests; target stop times.  Exact equality.
No GPU.
"""
import functools
import time

import numpy as np
import pytest

from boolsi_amd import synth
from boolsi_amd.attract import merge_tables
from boolsi_amd.compile import compile_problem
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text
from wide_ref import WideRef, aggregate, words_of

VARIATIONS_YAML = synth.network_yaml(40, 2, 77, initial={i: str(i & 1) for i in range(14, 40)},
                                     fixed={3: 'any?', 17: '0?', 21: 'any'},
                                     perturbations={5: {'1': '2, 6-7', 'any?': '9'}, 30: {'0?': '3'}})


def _constants(n, seed, any_nodes):
    bits = synth.seeded_bits(n, seed)
    return {i: ('any' if i in any_nodes else str(bits[i])) for i in range(n)}


N200_YAML = synth.network_yaml(200, 3, 200003,
                               initial=_constants(200, 21, {0, 63, 64, 65, 127, 128, 150, 191, 192, 199}),
                               fixed={130: '1?', 7: '0'}, perturbations={70: {'1': '2, 5'}, 195: {'0': '5', '1': '11'}})
N256_YAML = synth.network_yaml(256, 2, 256002,
                               initial=_constants(256, 22, {0, 31, 63, 64, 127, 128, 191, 192, 254, 255}))

CASES = [       # name, YAML, parse mode, [(first, count, max_t, max_len)]: the first three as test_gpu_wide_family.py
    ('k9_n24', synth.network_yaml(24, 9, 924), Mode.ATTRACT, [(0, 1 << 12, 2000, None), (12345, 3000, 50, 4)]),
    ('k12_n20', synth.network_yaml(20, 12, 2012), Mode.ATTRACT, [(0, 1 << 13, 5000, None)]),
    ('variations_n40', VARIATIONS_YAML, Mode.SIMULATE, [(0, 1 << 15, 4096, None), (123456, 5000, 12, 2),
                                                        (-40000, 40000, 4096, None)]),
    ('sched_fixed_n200', N200_YAML, Mode.SIMULATE, [(0, 1024, 400, None), (700, 1000, 30, 6)]),
    ('full_words_n256', N256_YAML, Mode.ATTRACT, [(0, 1024, 3000, None), (100, 900, 20, 3)]),
]
IDS = [c[0] for c in CASES]
TARGET_NODES = {'variations_n40': [3, 5, 17, 21, 30], 'full_words_n256': [0, 64, 128, 192, 255]}


@functools.lru_cache(maxsize=None)
def _setup(text, mode):
    """Parsed once per case (the rule text of the k = 12 network takes the YAML parser longer than both tests)."""
    from oracle.cpu_oracle import Oracle
    net, space = compile_problem(parse_input_text(text, 5000, mode))
    return net, space, Oracle(net, space), WideRef(net, space)


@pytest.mark.parametrize('name,text,mode,runs', CASES, ids=IDS)
def test_attract_equals_oracle(name, text, mode, runs):
    from oracle.cpu_oracle import key_int
    net, space, orc, ref = _setup(text, mode)
    for first, count, max_t, max_len in runs:
        first = first % space.n_problems
        pp, otable, onone, osteps = orc.attract(first, count, max_t, max_len, True, n_threads=8)
        t0 = time.perf_counter()
        recs, steps = ref.attract(range(first, first + count), max_t, max_len)
        print(name, first, count, 'reference seconds', round(time.perf_counter() - t0, 2))
        assert len(recs) == count
        expect = [(bool(r['found']), key_int(r['key']), int(r['length']), int(r['trajectory_l']), int(r['t_stop']))
                  for r in pp]
        assert recs == expect
        table, none = aggregate(recs)
        assert table == merge_tables([otable]) and none == onone and steps == osteps


@pytest.mark.parametrize('name,text,mode,runs', CASES, ids=IDS)
def test_simulate_and_target_equal_oracle(name, text, mode, runs):
    net, space, orc, ref = _setup(text, mode)
    count, max_t = min(3000, space.n_problems), 40
    # (variations_n40: 16384 problems per variant; the range takes in two of them)
    first = 5 * 16384 - 1500 if name == 'variations_n40' else min(4321 % space.n_problems, space.n_problems - count)
    otraj, ofinal, odigest, _ = orc.simulate(first, count, max_t)
    idx = range(first, first + count)
    traj, final, digest = ref.simulate(idx, max_t)
    W = net.n_words
    assert np.array_equal(np.array([[words_of(c, W) for c in tr] for tr in traj], np.uint64), otraj)
    assert np.array_equal(np.array([words_of(c, W) for c in final], np.uint64), ofinal)
    assert np.array_equal(np.array(digest, np.uint64), odigest)
    # trajectories of unequal lengths are prefixes of the same runs
    some = ref.trajectories([first + 9, first + 2, first + 30], [0, 17, 40])
    assert some == [traj[9][:1], traj[2][:18], traj[30][:41]]
    # target: a substate of five nodes (nodes that vary between the problems where the trajectories merge early), from
    # the first state, at or after the last perturbation, that some trajectories pass through and some do not
    nodes = TARGET_NODES.get(name, [1, 4, 7, 10, net.n_nodes - 1])
    mask = sum(1 << i for i in nodes)
    tp_max = max(ref.problem(i).tp for i in idx)
    codes = np.array([[c & mask for c in tr[tp_max:]] for tr in traj], object)
    code = next(c for c in dict.fromkeys(codes.ravel().tolist()) if 0 < (codes == c).any(axis=1).mean() < 1)
    for cap in (max_t, 11):
        pp, _ = orc.target(first, count, cap, np.array(words_of(mask, W), np.uint64),
                           np.array(words_of(code, W), np.uint64), n_threads=8)
        got = ref.target(idx, cap, nodes, code)
        assert got == [(bool(r['reached']), int(r['t_stop'])) for r in pp]
        assert cap < max_t or (any(g[0] for g in got) and not all(g[0] for g in got))
