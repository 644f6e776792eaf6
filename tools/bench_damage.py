"""
Damage spreading (DESIGN.md §3 "Damage spreading") next to the code it shares its step with: bsx_run_damage_sampled with
one flip on n = 300 and n = 1024 (every node 'any'), K = 2 and K = 4, against bsx_run_simulate_sampled over the same
samples and steps with final states only.  A damage call updates two states per sample, so the yardstick is TWICE the
simulate call's kernel_ms: existing code, doing the same 2 N T trajectory updates on the same build.

Protocol (that of tools/bench_sampled_target.py): every figure is the second of two calls in a fresh process; three
processes per variant, the variants alternated; min and max of kernel_ms are reported, the ratio from the minima.

    python tools/bench_damage.py [--count N] [--steps T] [--rounds R] > profiles/damage_spreading.json
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
            if call == 'damage':
                sum_d, _, merged, _, st = eng.damage_sampled(7, 0, count, 1, steps)
                extra = {'mean_d_1': int(sum_d[1]) / count, 'mean_d_T': int(sum_d[steps]) / count, 'merged_T': int(merged[steps]) / count}
            else:
                st = eng.simulate_sampled(7, 0, count, steps, trajectories=False, final=True, digest=False)[3]
    print(json.dumps(dict({'kernel_ms': st['kernel_ms'], 'total_ms': st['total_ms'], 'state_steps': st['state_steps'],
                           'executed_steps': st['executed_steps'], 'kernel_launches': st['kernel_launches']}, **extra)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--count', type=int, default=1 << 18)
    ap.add_argument('--steps', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--one', nargs=5, metavar=('CALL', 'N', 'K', 'COUNT', 'STEPS'), help='internal: one process of one variant')
    a = ap.parse_args()
    if a.one:
        return one(a.one[0], *(int(v) for v in a.one[1:]))
    variants = [(call,) + c for c in CASES for call in ('simulate', 'damage')]
    runs = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v in variants:                  # alternated: a drift of the device shows in every variant alike
            cmd = [sys.executable, os.path.abspath(__file__), '--one', v[0], str(v[1]), str(v[2]), str(a.count), str(a.steps)]
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                sys.exit('variant {} failed:\n{}'.format(v, res.stdout + res.stderr))
            runs[v].append(json.loads(res.stdout.splitlines()[-1]))
    out = []
    for n, k in CASES:
        sim, dam = runs[('simulate', n, k)], runs[('damage', n, k)]
        sim_ms = [min(r['kernel_ms'] for r in sim), max(r['kernel_ms'] for r in sim)]
        dam_ms = [min(r['kernel_ms'] for r in dam), max(r['kernel_ms'] for r in dam)]
        last = dam[-1]
        out.append({'n': n, 'k': k, 'count': a.count, 'steps': a.steps, 'flips': 1, 'processes': len(dam),
                    'simulate_kernel_ms': sim_ms, 'damage_kernel_ms': dam_ms, 'ratio_to_twice_simulate': dam_ms[0] / (2 * sim_ms[0]),
                    'state_steps': last['state_steps'], 'executed_steps': last['executed_steps'],
                    'executed_to_reference': last['executed_steps'] / last['state_steps'],
                    'mean_d_1': last['mean_d_1'], 'mean_d_T': last['mean_d_T'], 'merged_T': last['merged_T'],
                    'kernel_launches': last['kernel_launches']})
    print(json.dumps({'protocol': 'second of two calls in a fresh process; [min, max] over the processes; variants alternated; '
                                  'ratio = min damage kernel_ms / (2 * min simulate kernel_ms)', 'cases': out}, indent=1))


if __name__ == '__main__':
    main()
