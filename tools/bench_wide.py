"""
Wide-state family (DESIGN.md §3 "Wide networks"): executed node updates per second, one JSON line per case.
  simulate: fixed max_t, final states only;  attract: bsx_run_attract_wide over a sweep of 'any' initial states that
  spans several kernel launches, reduced on the device and, for comparison, on the host (BSX_WIDE_HOST_REDUCE=1);
  n = 128 forced through BSX_WIDE=1 next to the per-lane / k_simulate_sliced path the library picks by default.

    python tools/bench_wide.py [--count N] [--max-t T] [--attract-count N] [--attract-max-t T]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from boolsi_amd import synth                               # noqa: E402
from boolsi_amd.compile import compile_problem             # noqa: E402
from boolsi_amd.constants import Mode                      # noqa: E402
from boolsi_amd.engine import Engine                       # noqa: E402
from boolsi_amd.input import parse_input_text              # noqa: E402


def setup(eng, n, k, max_t, n_any=20):
    init = {i: ('any' if i < n_any else str(b)) for i, b in enumerate(synth.seeded_bits(n, n + k))}
    cfg = parse_input_text(synth.network_yaml(n, k, 1000 * n + k, initial=init), max_t, Mode.ATTRACT)
    net, space = compile_problem(cfg)
    eng.set_problem(net, space)
    return net


def timed(fn):
    fn()                                    # warm-up (module load, first-touch allocations)
    t0 = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    # (enough groups of 32 L trajectories for every CU of a 256-CU part: L = 16 at n = 300 / 512, 8 at 1024)
    ap.add_argument('--count', type=int, default=1 << 18)
    ap.add_argument('--max-t', type=int, default=256)
    ap.add_argument('--attract-count', type=int, default=1 << 20)      # four launches of 2^18 problems
    ap.add_argument('--attract-max-t', type=int, default=512)
    a = ap.parse_args()
    with Engine(0) as eng:
        for n in (300, 512, 1024):
            for k in (2, 3, 6):
                net = setup(eng, n, k, a.attract_max_t)
                info = eng.network_info()
                (_, _, _, st), wall = timed(lambda: eng.simulate(0, a.count, a.max_t, trajectories=False, digest=False))
                print(json.dumps({'case': 'simulate', 'n': n, 'k': k, 'count': a.count, 'max_t': a.max_t,
                                  'lut_mode': info['lut_mode'], 'kernel_ms': st['kernel_ms'],
                                  'node_updates_per_s': st['executed_steps'] * net.n_nodes / (st['kernel_ms'] * 1e-3),
                                  'wall_s': wall}), flush=True)
                for reduce in ('device', 'host'):
                    if reduce == 'host':
                        os.environ['BSX_WIDE_HOST_REDUCE'] = '1'
                    else:
                        os.environ.pop('BSX_WIDE_HOST_REDUCE', None)
                    r, wall = timed(lambda: eng.attract_wide(0, a.attract_count, a.attract_max_t))
                    st = r.stats
                    print(json.dumps({'case': 'attract', 'reduce': reduce, 'n': n, 'k': k, 'count': a.attract_count,
                                      'max_t': a.attract_max_t, 'attractors': len(r.table), 'none': r.n_no_attractor,
                                      'kernel_ms': st['kernel_ms'], 'total_ms': st['total_ms'],
                                      'host_syncs': st['host_syncs'], 'kernel_launches': st['kernel_launches'],
                                      'node_updates_per_s': st['executed_steps'] * net.n_nodes / (st['kernel_ms'] * 1e-3),
                                      'wall_s': wall}), flush=True)
                os.environ.pop('BSX_WIDE_HOST_REDUCE', None)
        for forced in (False, True):
            for k in (2, 3):
                if forced:
                    os.environ['BSX_WIDE'] = '1'
                else:
                    os.environ.pop('BSX_WIDE', None)
                net = setup(eng, 128, k, a.attract_max_t)
                (_, _, _, st), wall = timed(lambda: eng.simulate(0, a.count, a.max_t, trajectories=False, digest=False))
                print(json.dumps({'case': 'simulate_n128', 'k': k, 'family': 'wide' if forced else 'default',
                                  'lut_mode': eng.network_info()['lut_mode'], 'kernel_ms': st['kernel_ms'],
                                  'node_updates_per_s': st['executed_steps'] * net.n_nodes / (st['kernel_ms'] * 1e-3),
                                  'wall_s': wall}), flush=True)
        os.environ.pop('BSX_WIDE', None)


if __name__ == '__main__':
    main()
