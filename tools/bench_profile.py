#!/usr/bin/env python
"""
What the batched attractor profile (bsx_run_attractor_profile) buys over the per-attractor loop it replaces
(Engine.states_from: two problem-space uploads and a one-lane launch per attractor).  Two tables:

  identity   identity network, n = 16: 65 536 fixed points
  mixed      6 identity nodes + a 10-node LFSR: 64 fixed points and 64 cycles of 1023 states

For each: the batched call with activity only and with states (wall time of the call, kernel_ms of its launch, best of
--repeats), and the same table through the states_from loop.  For the identity table the loop is timed over a sample
of 1024 attractors and scaled to the table (the output says so).  One JSON line on stdout.

    python tools/bench_profile.py > profiles/attractor_profile.json          (needs the GPU)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from boolsi_amd import synth  # noqa: E402
from boolsi_amd.compile import compile_problem  # noqa: E402
from boolsi_amd.constants import Mode  # noqa: E402
from boolsi_amd.engine import Engine  # noqa: E402
from boolsi_amd.input import parse_input_text  # noqa: E402


def network_text(identity, lfsr, tap):
    n = len(identity) + len(lfsr)
    preds, masks = [[] for _ in range(n)], [0] * n
    for i in identity:
        preds[i], masks[i] = [i], 0b10
    if lfsr:
        preds[lfsr[0]], masks[lfsr[0]] = sorted((lfsr[-1], lfsr[tap - 1])), 0b0110
        for a, b in zip(lfsr, lfsr[1:]):
            preds[b], masks[b] = [a], 0b10
    out = ['nodes:'] + ['    - {}'.format(synth.node_name(i)) for i in range(n)] + ['', 'update rules:']
    out += ['    {}: {}'.format(synth.node_name(i), synth.rule_text(preds[i], masks[i])) for i in range(n)]
    out += ['', 'initial state:'] + ['    {}: any'.format(synth.node_name(i)) for i in range(n)]
    return '\n'.join(out) + '\n'


def tables():
    identity = ('identity', network_text(list(range(16)), [], 0), list(range(1 << 16)), [1] * (1 << 16), 1024)
    # the LFSR x^10 + x^7 + 1 on nodes 6 .. 15: state 1 (node 6 on) lies on its one cycle of 1023 states
    keys = [x | (lf << 6) for x in range(64) for lf in (1, 0)]
    lengths = [1023 if (k >> 6) else 1 for k in keys]
    mixed = ('mixed', network_text(list(range(6)), list(range(6, 16)), 7), keys, lengths, None)
    return identity, mixed


def best(fn, repeats):
    out = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        stats = fn()
        wall = (time.perf_counter() - t0) * 1e3
        if out is None or wall < out['wall_ms']:
            out = {'wall_ms': round(wall, 3), 'kernel_ms': round(stats['kernel_ms'], 4), 'kernel_launches': stats['kernel_launches']}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()
    result = {'tool': 'bench_profile', 'tables': {}}
    with Engine(0) as eng:
        result['device'] = eng.device_info()['name']
        for name, text, keys, lengths, sample in tables():
            net, space = compile_problem(parse_input_text(text, float('inf'), Mode.ATTRACT))
            eng.set_problem(net, space)

            def run(states):
                on, listed, closed = eng.attractor_profile(keys, lengths, states=states)
                assert closed.all()
                return eng.profile_stats

            run(True)                                                                     # warm-up: code objects, allocations
            row = {'attractors': len(keys), 'states': int(sum(lengths)),
                   'batched_activity_only': best(lambda: run(False), args.repeats),
                   'batched_with_states': best(lambda: run(True), args.repeats)}
            part = list(range(len(keys))) if sample is None else list(range(0, len(keys), len(keys) // sample))[:sample]
            eng.states_from(keys[0], lengths[0] - 1)
            t0 = time.perf_counter()
            for q in part:
                eng.states_from(keys[q], lengths[q] - 1)
            loop_ms = (time.perf_counter() - t0) * 1e3
            row['states_from_loop'] = {'attractors_timed': len(part), 'wall_ms': round(loop_ms, 3),
                                       'wall_ms_whole_table': round(loop_ms * len(keys) / len(part), 3),
                                       'scaled_from_sample': sample is not None}
            # the same states either way (checked on the timed part)
            _, listed, _ = eng.attractor_profile([keys[q] for q in part[:64]], [lengths[q] for q in part[:64]])
            assert all(np.array_equal(s, eng.states_from(keys[q], lengths[q] - 1)) for s, q in zip(listed, part[:64]))
            result['tables'][name] = row
    print(json.dumps(result))


if __name__ == '__main__':
    main()
