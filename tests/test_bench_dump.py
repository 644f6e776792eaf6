"""
bench.py --dump-outputs: what the last timed step returned, as float64 32-bit limbs (exact for 64-bit keys and wide
counts), the attractor rows in key order.  On the GPU the dump must equal the CPU oracle over the same index range.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from boolsi_amd import _lib
from boolsi_amd.engine import AttractResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def limbs_to_ints(a):
    """inverse of bench.u32_limbs along the last axis"""
    return [sum(int(x) << (32 * j) for j, x in enumerate(row)) for row in a.reshape(-1, a.shape[-1])]


def load_dump(path):
    return {f[:-len('.npy')]: np.load(os.path.join(path, f)) for f in os.listdir(path)}


def test_limbs_are_exact_for_wide_values():
    words = np.array([[0, 2 ** 64 - 1], [0x0123456789ABCDEF, (1 << 53) + 1]], dtype=np.uint64)
    a = bench.u32_limbs(words)
    assert a.dtype == np.float64 and a.shape == (2, 4)
    assert limbs_to_ints(a) == [(2 ** 64 - 1) << 64, 0x0123456789ABCDEF | ((1 << 53) + 1) << 64]
    assert limbs_to_ints(bench.u32_limbs(2 ** 127 + 5)) == [2 ** 127 + 5]
    assert bench.u32_limbs(np.zeros((0, 4), np.uint64)).shape == (0, 8)


def test_dump_outputs_sorts_rows_by_key(tmp_path):
    t = np.zeros(3, _lib.ATTR_REC2)
    t['key'][:, 0] = [7, 3, 5]
    t['key'][2, 1] = 1                              # 5 + 2^64: the largest key
    t['length'] = [1, 2, 3]
    t['count'][:, 0] = [10, 20, 30]
    t['count'][0, 1] = 1
    t['sum_l2'][1, 3] = 9
    bench.dump_outputs(str(tmp_path), AttractResult(t, 2 ** 70 + 1, None, {'state_steps': 2 ** 65 + 3}))
    got = load_dump(tmp_path)
    assert sorted(got) == sorted(['attractor_' + f for f in _lib.ATTR_REC2.names] + ['n_no_attractor', 'state_steps'])
    assert all(a.dtype == np.float64 for a in got.values())
    assert limbs_to_ints(got['attractor_key']) == [3, 7, 5 + 2 ** 64]
    assert limbs_to_ints(got['attractor_length']) == [2, 1, 3]
    assert limbs_to_ints(got['attractor_count']) == [20, 10 + 2 ** 64, 30]
    assert limbs_to_ints(got['attractor_sum_l2']) == [9 << 192, 0, 0]
    assert limbs_to_ints(got['n_no_attractor']) == [2 ** 70 + 1]
    assert limbs_to_ints(got['state_steps']) == [2 ** 65 + 3]


def test_steps_below_one_are_refused():
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], cwd=ROOT, capture_output=True,
                         text=True, timeout=60)
    assert res.returncode != 0 and '--steps' in res.stderr


@pytest.mark.gpu
def test_dump_is_the_last_timed_step_and_equals_the_oracle(tmp_path):
    from boolsi_amd import synth
    from boolsi_amd.compile import compile_problem
    from boolsi_amd.constants import Mode
    from boolsi_amd.input import parse_input_text
    from oracle.cpu_oracle import Oracle

    log2_batch, warmup, steps = 16, 1, 3
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', str(steps), '--warmup', str(warmup),
           '--log2-batch', str(log2_batch), '--no-cpu-baseline', '--dump-outputs', str(tmp_path / 'out')]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert json.loads(res.stdout.strip().splitlines()[-1])['steps'] == steps
    got = load_dump(tmp_path / 'out')

    # the index range of step number warmup + steps - 1, pinned here: the dump's inputs must not move between builds
    batch = 1 << log2_batch
    first = (0x0123456789ABCDEF & ~(batch - 1)) + (warmup + steps - 1) * batch
    net, space = compile_problem(parse_input_text(synth.north_star_yaml(), bench.MAX_T, Mode.ATTRACT))
    _, table, none, state_steps = Oracle(net, space).attract(first, batch, bench.MAX_T, per_problem=False, n_threads=os.cpu_count())
    table = sorted(table.tolist(), key=lambda a: [int(w) for w in reversed(a[0])])
    assert len(table) > 0
    assert limbs_to_ints(got['attractor_key']) == [sum(int(w) << (64 * i) for i, w in enumerate(a[0])) for a in table]
    assert limbs_to_ints(got['attractor_length']) == [a[1] for a in table]
    assert limbs_to_ints(got['attractor_count']) == [a[2] for a in table]
    assert limbs_to_ints(got['attractor_sum_l']) == [a[3] for a in table]
    assert limbs_to_ints(got['attractor_sum_l2']) == [a[4] | a[5] << 64 for a in table]
    assert limbs_to_ints(got['n_no_attractor']) == [none]
    assert limbs_to_ints(got['state_steps']) == [state_steps]
