#!/usr/bin/env python
"""
Node correlations of a whole attractor table: the host path (one device call for the on-counts, then numpy: a sort per
node column and np.cov) against the device path (Engine.node_correlations -> bsx_run_node_correlations), both from
(keys, lengths, frequencies) to (Rho, P) through attractor_analysis.correlation_statistics.

Tables: fixed points of an identity network of 64 and of 1024 nodes, random distinct keys, frequencies 1 .. 100, at
2^12, 2^16, 2^20 and 2^24 cells (attractors x nodes).  Per table one untimed call of each path first (code objects,
allocations), then three runs of each, alternated.  The two paths' Rho must agree within 1e-9 with the same NaN
pattern.  `crossover_cells` is the smallest measured size from which on every device run beats every host run at both
widths; attractor_analysis.DEVICE_CORRELATION_CELLS is set from it (not below 2^12).  One JSON line on stdout.

    python tools/bench_correlations.py > profiles/node_correlations.json          (needs the GPU)
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from boolsi_amd import synth  # noqa: E402
from boolsi_amd.attractor_analysis import compute_frequency_spearmanrho, correlation_statistics  # noqa: E402
from boolsi_amd.compile import compile_problem  # noqa: E402
from boolsi_amd.constants import Mode  # noqa: E402
from boolsi_amd.engine import Engine  # noqa: E402
from boolsi_amd.input import parse_input_text  # noqa: E402

CELLS = (1 << 12, 1 << 16, 1 << 20, 1 << 24)
WIDTHS = (64, 1024)


def identity_text(n):
    out = ['nodes:'] + ['    - {}'.format(synth.node_name(i)) for i in range(n)] + ['', 'update rules:']
    out += ['    {}: {}'.format(synth.node_name(i), synth.rule_text([i], 0b10)) for i in range(n)]
    out += ['', 'initial state:'] + ['    {}: {}'.format(synth.node_name(i), 'any' if i < 8 else '0') for i in range(n)]
    return '\n'.join(out) + '\n'


def table(n_nodes, count, seed):
    rng = random.Random(seed)
    keys = set()
    while len(keys) < count:
        keys.add(rng.getrandbits(n_nodes))
    keys = list(keys)
    return keys, [1] * count, [rng.randint(1, 100) for _ in range(count)]


def host_path(eng, keys, lengths, freq):
    on, _, closed = eng.attractor_profile(keys, lengths, states=False)
    assert closed.all()
    obs = on.astype(np.float64) / np.asarray(lengths, np.float64)[:, None]
    return compute_frequency_spearmanrho(obs, np.array(freq))


def device_path(eng, keys, lengths, freq):
    S, _, _, closed = eng.node_correlations(keys, lengths, freq)
    assert closed.all()
    return correlation_statistics(S, sum(freq) - 2)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--max-cells', type=int, default=CELLS[-1])
    args = ap.parse_args()
    result = {'tool': 'bench_correlations', 'runs': args.runs, 'tables': []}
    with Engine(0) as eng:
        result['device'] = eng.device_info()['name']
        for n_nodes in WIDTHS:
            net, space = compile_problem(parse_input_text(identity_text(n_nodes), float('inf'), Mode.ATTRACT))
            eng.set_problem(net, space)
            for cells in CELLS:
                if cells > args.max_cells:
                    continue
                count = cells // n_nodes
                keys, lengths, freq = table(n_nodes, count, cells + n_nodes)
                (rho_h, _), _ = timed(lambda: host_path(eng, keys, lengths, freq))         # untimed first calls
                (rho_d, _), _ = timed(lambda: device_path(eng, keys, lengths, freq))
                assert np.array_equal(np.isnan(rho_h), np.isnan(rho_d))
                ok = ~np.isnan(rho_h)
                diff = float(np.max(np.abs(rho_h[ok] - rho_d[ok]))) if ok.any() else 0.0
                assert diff <= 1e-9, diff
                host_ms, device_ms, kernel_ms = [], [], []
                for _ in range(args.runs):
                    host_ms.append(round(timed(lambda: host_path(eng, keys, lengths, freq))[1], 3))
                    device_ms.append(round(timed(lambda: device_path(eng, keys, lengths, freq))[1], 3))
                    kernel_ms.append(round(eng.corr_stats['kernel_ms'], 4))
                result['tables'].append({'n_nodes': n_nodes, 'attractors': count, 'cells': cells, 'host_ms': host_ms,
                                         'device_ms': device_ms, 'device_kernel_ms': kernel_ms,
                                         'device_kernel_launches': eng.corr_stats['kernel_launches'],
                                         'max_abs_rho_difference': diff,
                                         'device_wins': max(device_ms) < min(host_ms)})
                print('{} nodes x {} attractors: host {} ms, device {} ms'.format(n_nodes, count, host_ms, device_ms),
                      file=sys.stderr, flush=True)
    crossover = None
    for cells in sorted({t['cells'] for t in result['tables']}, reverse=True):
        if all(t['device_wins'] for t in result['tables'] if t['cells'] >= cells):
            crossover = cells
    result['crossover_cells'] = crossover
    print(json.dumps(result))


if __name__ == '__main__':
    main()
