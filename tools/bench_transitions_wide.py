#!/usr/bin/env python
"""
Single-node flip transitions of a whole attractor table on the wide-state family: the device call
(Engine.attractor_transitions_wide -> bsx_run_attractor_transitions_wide) against what there was before it for
networks of more than 256 nodes, a host loop of one set_space + attract_wide(0, 1) per flip with the flipped state as
the origin.

Tables: K = 2 random networks (synth.random_network) of 300, 577 and 1024 nodes, the first 8 nodes 'any'; the rows are
the attractors attract_wide finds from the 256 initial states, in key order, as many as stay within `--states` cycle
states.  Per table one untimed device call first (code objects, allocations), then `--runs` timed ones: wall time of
the call and the kernel time of its statistics; the median is reported.  The loop is timed on a SAMPLE of `--sample`
flips spread evenly over the table (after 4 untimed ones) and scaled to the whole table, which the output says; every
sampled flip's destination must be an edge of the device call.  `walk_share`: the kernel time of a second call with
max_t = 0 (every phase but the mu pass and the key lap still runs for two lock steps) against the full call's.
One JSON line.

    python tools/bench_transitions_wide.py > profiles/attractor_transitions_wide.json          (needs the GPU)
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

from boolsi_amd import _lib, synth  # noqa: E402
from boolsi_amd.compile import code_to_words, compile_problem, words_to_code  # noqa: E402
from boolsi_amd.constants import Mode  # noqa: E402
from boolsi_amd.engine import Engine  # noqa: E402
from boolsi_amd.input import parse_input_text  # noqa: E402

N_ANY = 8


def network_text(n, seed):
    preds, masks = synth.random_network(n, 2, seed)
    bits = synth.seeded_bits(n, seed + 3)
    out = ['nodes:'] + ['    - {}'.format(synth.node_name(i)) for i in range(n)] + ['', 'update rules:']
    out += ['    {}: {}'.format(synth.node_name(i), synth.rule_text(preds[i], masks[i])) for i in range(n)]
    out += ['', 'initial state:'] + ['    {}: {}'.format(synth.node_name(i), 'any' if i < N_ANY else bits[i]) for i in range(n)]
    return '\n'.join(out) + '\n'


def found_table(eng, budget):
    r = eng.attract_wide(0, 1 << N_ANY)
    rows = sorted((int(words_to_code(rec['key'])), int(rec['length'])) for rec in r.table)
    keys, lengths, total = [], [], 0
    for k, l in rows:
        if total + l > budget:
            continue
        keys.append(k); lengths.append(l); total += l
    return keys, lengths, len(rows)


def loop_flip(eng, net, space, x0):
    """the flip as its own problem: -> key of its attractor"""
    eng.set_space(dataclasses.replace(space, origin_state=code_to_words(x0, net.n_words), any_nodes=np.zeros(0, np.uint32),
                                      n_problems=1, radices=[]))
    r = eng.attract_wide(0, 1)
    assert len(r.table) == 1
    return int(words_to_code(r.table[0]['key']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--sample', type=int, default=128)
    ap.add_argument('--states', type=int, default=4096)
    ap.add_argument('--seeds', type=int, nargs=3, default=[0, 16, 3], help='seeds of the 300-, 577- and 1024-node networks')
    args = ap.parse_args()
    result = {'tool': 'bench_transitions_wide', 'runs': args.runs, 'loop_sample_flips': args.sample,
              'loop_note': 'loop_ms_scaled = per-flip median of the sampled loop x number of flips; the loop was not run in full',
              'tables': []}
    with Engine(0) as eng:
        result['device'] = eng.device_info()['name']
        for n, seed in zip((300, 577, 1024), args.seeds):
            net, space = compile_problem(parse_input_text(network_text(n, seed), float('inf'), Mode.ATTRACT))
            eng.set_problem(net, space)
            assert eng.wide
            keys, lengths, found = found_table(eng, args.states)
            if not keys:
                print('n = {}: no attractor within the budget of cycle states'.format(n), file=sys.stderr)
                continue
            n_states, n_free = sum(lengths), net.n_nodes
            edges, _, closed = eng.attractor_transitions_wide(keys, lengths)            # untimed first call
            assert closed.all()
            wall, kernel, idle = [], [], []
            for _ in range(args.runs):
                t0 = time.perf_counter()
                again, _, _ = eng.attractor_transitions_wide(keys, lengths)
                wall.append((time.perf_counter() - t0) * 1e3)
                kernel.append(eng.trans_stats['kernel_ms'])
                stats = dict(eng.trans_stats)
                assert np.array_equal(again, edges)
                eng.attractor_transitions_wide(keys, lengths, max_t=0)
                idle.append(eng.trans_stats['kernel_ms'])
            # the loop, on a sample of the flips
            states = eng.attractor_profile(keys, lengths, activity=False)[1]
            flat = [(q, int(words_to_code(s))) for q, rows in enumerate(states) for s in rows]
            flips = n_states * n_free
            picks = [int(i * flips / args.sample) for i in range(min(args.sample, flips))]
            per_flip, row_of = [], {k: q for q, k in enumerate(keys)}
            want = {(int(e['src']), int(e['dst'])) for e in edges}
            for at, f in enumerate([0] * 4 + picks):
                q, s = flat[f // n_free]
                t0 = time.perf_counter()
                key = loop_flip(eng, net, space, s ^ (1 << (f % n_free)))
                if at >= 4:
                    per_flip.append((time.perf_counter() - t0) * 1e3)
                assert (q, row_of.get(key, _lib.TRANS_OUTSIDE)) in want
            eng.set_space(space)
            med = statistics.median
            result['tables'].append({
                'n_nodes': n, 'seed': seed, 'attractors_found': found, 'attractors': len(keys), 'cycle_states': n_states, 'flips': flips,
                'edges': len(edges), 'sum_mu': stats['state_steps'], 'executed_steps': stats['executed_steps'],
                'kernel_launches': stats['kernel_launches'],
                'device_wall_ms_median': round(med(wall), 4), 'device_wall_ms': [round(x, 4) for x in wall],
                'device_kernel_ms_median': round(med(kernel), 4), 'device_kernel_ms': [round(x, 4) for x in kernel],
                'kernel_ms_at_max_t_0_median': round(med(idle), 4),
                'walk_share': round(1 - med(idle) / med(kernel), 3),
                'loop_ms_per_flip_median': round(med(per_flip), 4), 'loop_ms_scaled': round(med(per_flip) * flips, 1),
                'speedup_wall': round(med(per_flip) * flips / med(wall), 1)})
            print(result['tables'][-1], file=sys.stderr, flush=True)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
