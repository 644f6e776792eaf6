"""
Target over sampled initial conditions next to the enumerating summary call: bsx_run_target_sampled with
cap = 0 (count and histogram only, one host wait) on n = 300 (20 'any' nodes), n = 577 (300 'any' nodes) and n = 1024
(every node 'any'), K = 2, and on n = 300 bsx_run_target_summary over as many consecutive problems.  The enumerating code
is the baseline: the two differ in a group's set-up only.

Protocol (that of tools/bench_sampled.py): every figure is the second of two calls in a fresh process; three processes per
variant, the variants alternated; min and max of kernel_ms and total_ms are reported.  The target substate is the state
of five nodes in the origin state with the first of them inverted.

    python tools/bench_sampled_target.py [--count N] [--max-t T] [--rounds R] > profiles/target_sampled.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((300, 20), (577, 300), (1024, 1024))       # (nodes, 'any' nodes)


def one(source, n, n_any, count, max_t):
    from boolsi_amd import synth
    from boolsi_amd.compile import code_to_words, compile_problem
    from boolsi_amd.constants import Mode
    from boolsi_amd.engine import Engine
    from boolsi_amd.input import parse_input_text
    bits = synth.seeded_bits(n, n + 2)
    init = {i: ('any' if i < n_any else str(b)) for i, b in enumerate(bits)}
    net, space = compile_problem(parse_input_text(synth.network_yaml(n, 2, 1000 * n + 2, initial=init), max_t, Mode.ATTRACT))
    nodes = [n - 1, n - 40, n // 2, 100, 5]
    mask = code_to_words(sum(1 << i for i in nodes), net.n_words)
    code = code_to_words(sum((int(bits[i]) ^ (i == nodes[0])) << i for i in nodes), net.n_words)
    with Engine(0) as eng:
        eng.set_problem(net, space)
        for _ in range(2):
            if source == 'sampled':
                n_hits, hist, _, st = eng.target_sampled(7, 0, count, max_t, mask, code, hist_bins=64, cap=0)
            else:
                n_hits, hist, _, st = eng.target_summary(0, count, max_t, mask, code, hist_bins=64, cap=0)
    print(json.dumps({'kernel_ms': st['kernel_ms'], 'total_ms': st['total_ms'], 'hits': int(n_hits), 'state_steps': st['state_steps'],
                      'executed_steps': st['executed_steps'], 'kernel_launches': st['kernel_launches']}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--count', type=int, default=1 << 20)
    ap.add_argument('--max-t', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--one', nargs=5, metavar=('SOURCE', 'N', 'N_ANY', 'COUNT', 'MAX_T'), help='internal: one process of one variant')
    a = ap.parse_args()
    if a.one:
        return one(a.one[0], *(int(v) for v in a.one[1:]))
    variants = [('enumerated',) + CASES[0]] + [('sampled',) + c for c in CASES]
    runs = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v in variants:                  # alternated: a drift of the device shows in every variant alike
            cmd = [sys.executable, os.path.abspath(__file__), '--one', v[0], str(v[1]), str(v[2]), str(a.count), str(a.max_t)]
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                sys.exit('variant {} failed:\n{}'.format(v, res.stdout + res.stderr))
            runs[v].append(json.loads(res.stdout.splitlines()[-1]))
    out = []
    for (source, n, n_any), rs in runs.items():
        out.append({'source': source, 'n': n, 'k': 2, 'n_any': n_any, 'count': a.count, 'max_t': a.max_t, 'processes': len(rs),
                    'kernel_ms': [min(r['kernel_ms'] for r in rs), max(r['kernel_ms'] for r in rs)],
                    'total_ms': [min(r['total_ms'] for r in rs), max(r['total_ms'] for r in rs)],
                    'hits': rs[-1]['hits'], 'state_steps': rs[-1]['state_steps'], 'executed_steps': rs[-1]['executed_steps'],
                    'kernel_launches': rs[-1]['kernel_launches']})
    print(json.dumps({'protocol': 'second of two calls in a fresh process; [min, max] over the processes; variants alternated',
                      'cases': out}, indent=1))


if __name__ == '__main__':
    main()
