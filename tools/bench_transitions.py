#!/usr/bin/env python
"""
Single-node flip transitions of a whole attractor table: the device call (Engine.attractor_transitions ->
bsx_run_attractor_transitions) against the only way there was before it, a host loop of one set_space + attract(0, 1)
per flip with the flipped state as the origin.

Tables:
  mixed      16 nodes (6 identity nodes + a 10-node LFSR), 128 attractors of lengths 1 and 1023: 65 536 cycle states,
             2^20 flips, every one of them on a listed cycle at once (mu = 0): the walk is one table probe per flip
  mixed_half the same network with every other row of that table: the flips that used to reach a missing row now end on an
             unlisted 1023-cycle, which Brent's detector and the mu pass walk for some 4 000 steps, each detector step
             with a probe that misses
  north_star the n = 64, K = 2 network of the benchmark, the attractors found from 2^16 initial states: few cycle
             states, flips that run for some steps before they meet a listed state (a probe per step)
Per table one untimed device call first (code objects, allocations), then `--runs` timed ones: wall time of the call and
the kernel time of its statistics; the median is reported.  The loop is timed on a SAMPLE of `--sample` flips spread
evenly over the table (after 8 untimed ones) and scaled to the whole table, which the output says; the sampled flips'
destinations and recovery times must add up to the device call's edges over that sample's rows where the sample is
the whole table.  `walk_share`: the kernel time of a second call with max_t = 0, which loads and books every flip but takes no step and
makes no probe (what the profile, the table build, the launches, the edge tables and the drain cost), against the full
call's; on `mixed`, where no flip takes a step, the difference is the probes alone.  One JSON line.

    python tools/bench_transitions.py > profiles/attractor_transitions.json          (needs the GPU)
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from boolsi_amd import synth  # noqa: E402
from boolsi_amd.compile import code_to_words, compile_problem, words_to_code  # noqa: E402
from boolsi_amd.constants import Mode  # noqa: E402
from boolsi_amd.engine import Engine  # noqa: E402
from boolsi_amd.input import parse_input_text  # noqa: E402


def mixed_text():
    n, identity, lfsr, tap = 16, list(range(6)), list(range(6, 16)), 7
    preds, masks = [[] for _ in range(n)], [0] * n
    for i in identity:
        preds[i], masks[i] = [i], 0b10
    a, b = sorted((lfsr[-1], lfsr[tap - 1]))
    preds[lfsr[0]], masks[lfsr[0]] = [a, b], 0b0110
    for i in range(1, len(lfsr)):
        preds[lfsr[i]], masks[lfsr[i]] = [lfsr[i - 1]], 0b10
    out = ['nodes:'] + ['    - {}'.format(synth.node_name(i)) for i in range(n)] + ['', 'update rules:']
    out += ['    {}: {}'.format(synth.node_name(i), synth.rule_text(preds[i], masks[i])) for i in range(n)]
    out += ['', 'initial state:'] + ['    {}: any'.format(synth.node_name(i)) for i in range(n)]
    return '\n'.join(out) + '\n'


def found_table(eng, count):
    r = eng.attract(0, count)
    rows = sorted((int(words_to_code(rec['key'])), int(rec['length'])) for rec in r.table)
    return [k for k, _ in rows], [l for _, l in rows]


def loop_flip(eng, net, space, x0):
    """the flip as its own problem: -> (key, length, mu)"""
    eng.set_space(dataclasses.replace(space, origin_state=code_to_words(x0, net.n_words), any_nodes=np.zeros(0, np.uint32),
                                      n_problems=1, radices=[]))
    r = eng.attract(0, 1, per_problem=True)
    p = r.per_problem[0]
    assert p['found']
    return int(words_to_code(p['key'])), int(p['length']), int(p['trajectory_l'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--sample', type=int, default=512)
    args = ap.parse_args()
    result = {'tool': 'bench_transitions', 'runs': args.runs, 'loop_sample_flips': args.sample,
              'loop_note': 'loop_ms_scaled = per-flip median of the sampled loop x number of flips; the loop was not run in full',
              'tables': []}
    with Engine(0) as eng:
        result['device'] = eng.device_info()['name']
        for name, text, every in (('mixed', mixed_text(), 1), ('mixed_half', mixed_text(), 2), ('north_star', synth.north_star_yaml(), 1)):
            net, space = compile_problem(parse_input_text(text, float('inf'), Mode.ATTRACT))
            eng.set_problem(net, space)
            keys, lengths = found_table(eng, 1 << 16)
            keys, lengths = keys[::every], lengths[::every]
            n_states, n_free = sum(lengths), net.n_nodes
            edges, _, closed = eng.attractor_transitions(keys, lengths)                 # untimed first call
            assert closed.all()
            wall, kernel, idle = [], [], []
            for _ in range(args.runs):
                t0 = time.perf_counter()
                again, _, _ = eng.attractor_transitions(keys, lengths)
                wall.append((time.perf_counter() - t0) * 1e3)
                kernel.append(eng.trans_stats['kernel_ms'])
                stats = dict(eng.trans_stats)
                assert np.array_equal(again, edges)
                eng.attractor_transitions(keys, lengths, max_t=0)
                idle.append(eng.trans_stats['kernel_ms'])
            # the loop, on a sample of the flips
            states = eng.attractor_profile(keys, lengths, activity=False)[1]
            flat = [(q, int(words_to_code(s))) for q, rows in enumerate(states) for s in rows]
            flips = n_states * n_free
            picks = [int(i * flips / args.sample) for i in range(min(args.sample, flips))]
            per_flip, row_of = [], {k: q for q, k in enumerate(keys)}
            want = {(int(e['src']), int(e['dst'])) for e in edges}
            for at, f in enumerate([0] * 8 + picks):
                q, s = flat[f // n_free]
                t0 = time.perf_counter()
                key, _, _ = loop_flip(eng, net, space, s ^ (1 << (f % n_free)))
                if at >= 8:
                    per_flip.append((time.perf_counter() - t0) * 1e3)
                assert (q, row_of.get(key, 0xFFFFFFFE)) in want
            eng.set_space(space)
            med = statistics.median
            result['tables'].append({
                'table': name, 'n_nodes': net.n_nodes, 'attractors': len(keys), 'cycle_states': n_states, 'flips': flips,
                'edges': len(edges), 'sum_mu': stats['state_steps'], 'executed_steps': stats['executed_steps'],
                'kernel_launches': stats['kernel_launches'],
                'device_wall_ms_median': round(med(wall), 4), 'device_wall_ms': [round(x, 4) for x in wall],
                'device_kernel_ms_median': round(med(kernel), 4), 'device_kernel_ms': [round(x, 4) for x in kernel],
                'kernel_ms_without_walks_median': round(med(idle), 4),
                'walk_share': round(1 - med(idle) / med(kernel), 3),
                'loop_ms_per_flip_median': round(med(per_flip), 4), 'loop_ms_scaled': round(med(per_flip) * flips, 1),
                'speedup_wall': round(med(per_flip) * flips / med(wall), 1)})
            print(result['tables'][-1], file=sys.stderr, flush=True)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
