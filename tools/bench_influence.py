"""
The influence matrix (DESIGN.md §3 "Node influence") next to the code it shares its step with: bsx_run_influence_sampled
with every node a source on n = 300 and n = 1024 (every node 'any'), K = 2 and K = 4, T = 16, against
bsx_run_simulate_sampled with final states only.  An influence call updates two states per (source, sample), so the
yardstick is 2 * n_sources times the simulate call's kernel_ms over the same samples and steps: existing code, doing the
same number of trajectory updates on the same build.  A simulate call over so few samples leaves most of the device idle,
so a second yardstick is given beside it: the same number of updates at the rate of a simulate call over --fill samples,
which fills the device.

Protocol (that of tools/bench_damage.py): every figure is the second of two calls in a fresh process; three processes per
variant, the variants alternated; min and max of kernel_ms are reported, the ratios from the minima.

    python tools/bench_influence.py [--count N] [--steps T] [--rounds R] > profiles/node_influence.json

BSX_LIB selects the library as everywhere; --libs NAME,NAME.. measures the influence call on further builds of the library
(the count stage compiled out, or built the other way: bsx_wide.hip, BSX_INFLUENCE_COUNTS) and reports their kernel_ms
beside the default build's.  Such a build is the Makefile's with EXTRA and OUT, as for the diagnostic library:
    make -C boolsi_amd/csrc EXTRA=-DBSX_INFLUENCE_COUNTS=0 OUT=../libbsx_hip_counts0.so     (then `make clean` and the default)
    python tools/bench_influence.py --libs libbsx_hip_counts0.so,libbsx_hip_counts1.so
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((300, 2), (300, 4), (1024, 2), (1024, 4))      # (nodes, K)


def one(call, n, k, count, steps):
    from boolsi_amd import synth
    from boolsi_amd.compile import compile_problem
    from boolsi_amd.constants import Mode
    from boolsi_amd.engine import Engine
    from boolsi_amd.input import parse_input_text
    init = {i: 'any' for i in range(n)}
    net, space = compile_problem(parse_input_text(synth.network_yaml(n, k, 1000 * n + k, initial=init), steps, Mode.ATTRACT))
    extra = {}
    with Engine(0) as eng:
        eng.set_problem(net, space)
        for _ in range(2):
            if call == 'influence':
                table, merged, st = eng.influence_sampled(7, 0, count, list(range(n)), steps)
                first = sum(int(v) for row in table[:, 0] for v in row)
                extra = {'average_sensitivity': first / (count * n), 'merged_T': int(merged[:, -1].sum()) / (count * n),
                         'dead_at_1': int((merged[:, 0] == count).sum())}
            else:
                st = eng.simulate_sampled(7, 0, count, steps, trajectories=False, final=True, digest=False)[3]
    print(json.dumps(dict({'kernel_ms': st['kernel_ms'], 'total_ms': st['total_ms'], 'state_steps': st['state_steps'],
                           'executed_steps': st['executed_steps'], 'kernel_launches': st['kernel_launches']}, **extra)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--count', type=int, default=1 << 13)
    ap.add_argument('--fill', type=int, default=1 << 18)
    ap.add_argument('--steps', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--libs', default='', help='further builds of the library to time the influence call on, comma-separated')
    ap.add_argument('--one', nargs=5, metavar=('CALL', 'N', 'K', 'COUNT', 'STEPS'), help='internal: one process of one variant')
    a = ap.parse_args()
    if a.one:
        return one(a.one[0], *(int(v) for v in a.one[1:]))
    libs = [name for name in a.libs.split(',') if name]
    variants = []
    for c in CASES:
        variants += [('simulate', None, a.count) + c, ('simulate', None, a.fill) + c, ('influence', None, a.count) + c]
        variants += [('influence', lib, a.count) + c for lib in libs]
    runs = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v in variants:                  # alternated: a drift of the device shows in every variant alike
            call, lib, count, n, k = v
            cmd = [sys.executable, os.path.abspath(__file__), '--one', call, str(n), str(k), str(count), str(a.steps)]
            env = dict(os.environ, BSX_LIB=lib) if lib else None
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
            if res.returncode != 0:
                sys.exit('variant {} failed:\n{}'.format(v, res.stdout + res.stderr))
            runs[v].append(json.loads(res.stdout.splitlines()[-1]))
            print('{} {}: {:.3f} ms'.format(v, len(runs[v]), runs[v][-1]['kernel_ms']), file=sys.stderr, flush=True)

    def span(rs):
        return [min(r['kernel_ms'] for r in rs), max(r['kernel_ms'] for r in rs)]

    out = []
    for n, k in CASES:
        sim, fill, inf = (runs[(call, None, count, n, k)] for call, count in (('simulate', a.count), ('simulate', a.fill), ('influence', a.count)))
        sim_ms, fill_ms, inf_ms = span(sim), span(fill), span(inf)
        last = inf[-1]
        case = {'n': n, 'k': k, 'count': a.count, 'steps': a.steps, 'sources': n, 'processes': len(inf),
                'simulate_kernel_ms': sim_ms, 'simulate_fill_count': a.fill, 'simulate_fill_kernel_ms': fill_ms,
                'influence_kernel_ms': inf_ms,
                'yardstick_ms': 2 * n * sim_ms[0], 'ratio_to_yardstick': inf_ms[0] / (2 * n * sim_ms[0]),
                'filled_yardstick_ms': 2 * n * fill_ms[0] * a.count / a.fill,
                'ratio_to_filled_yardstick': inf_ms[0] / (2 * n * fill_ms[0] * a.count / a.fill),
                'state_steps': last['state_steps'], 'executed_steps': last['executed_steps'],
                'executed_to_reference': last['executed_steps'] / last['state_steps'],
                'average_sensitivity': last['average_sensitivity'], 'merged_T': last['merged_T'], 'dead_at_1': last['dead_at_1'],
                'kernel_launches': last['kernel_launches']}
        for lib in libs:
            case['influence_kernel_ms ' + lib] = span(runs[('influence', lib, a.count, n, k)])
        out.append(case)
    print(json.dumps({'protocol': 'second of two calls in a fresh process; [min, max] over the processes; variants alternated; '
                                  'yardstick = 2 * sources * min simulate kernel_ms over the same samples and steps; filled yardstick = the '
                                  'same updates at the rate of a simulate call over simulate_fill_count samples; ratios from the minima',
                      'cases': out}, indent=1))


if __name__ == '__main__':
    main()
