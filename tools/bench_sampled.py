"""
Attract over sampled initial conditions next to the enumerating call on the same networks: the
networks of tools/bench_wide.py (n = 300 and 1024, K = 2, 20 'any' nodes), 2^20 samples against 2^20 consecutive
problems, plus n = 1024 with every node 'any', which has no enumerated counterpart.

Protocol: every figure is the second of two calls in a fresh process; three processes per variant, the variants
alternated; min and max of kernel_ms and total_ms are reported.  max_t = 1 leaves a handful of lock steps per group, so
the kernel_ms difference between the two sources there is the cost of the group set-up.
--parent-tree DIR adds the enumerating call of another build of the project (a built checkout of the parent commit) as
source "enumerated_parent", alternated with the others, to show that call has not moved.

    python tools/bench_sampled.py [--count N] [--max-t T] [--rounds R] [--parent-tree DIR] > profiles/attract_sampled.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (a --one child of the parent baseline imports the package of that tree instead)
sys.path.insert(0, os.environ.get('BSX_BENCH_TREE') or ROOT)


def one(source, n, n_any, count, max_t):
    from boolsi_amd import synth
    from boolsi_amd.compile import compile_problem
    from boolsi_amd.constants import Mode
    from boolsi_amd.engine import Engine
    from boolsi_amd.input import parse_input_text
    init = {i: ('any' if i < n_any else str(b)) for i, b in enumerate(synth.seeded_bits(n, n + 2))}
    net, space = compile_problem(parse_input_text(synth.network_yaml(n, 2, 1000 * n + 2, initial=init), max_t, Mode.ATTRACT))
    with Engine(0) as eng:
        eng.set_problem(net, space)
        for _ in range(2):
            # (cap: a sample of a large space may end in many attractors; the device structures follow min(cap, count))
            r = eng.attract_sampled(7, 0, count, max_t, cap=1 << 20) if source == 'sampled' else eng.attract_wide(0, count, max_t, cap=1 << 20)
    st = r.stats
    print(json.dumps({'kernel_ms': st['kernel_ms'], 'total_ms': st['total_ms'], 'attractors': len(r.table),
                      'none': r.n_no_attractor, 'executed_steps': st['executed_steps'], 'host_syncs': st['host_syncs']}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--count', type=int, default=1 << 20)
    ap.add_argument('--max-t', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent-tree', metavar='DIR', help='a built checkout of the parent commit: its bsx_run_attract_wide as a baseline')
    ap.add_argument('--one', nargs=5, metavar=('SOURCE', 'N', 'N_ANY', 'COUNT', 'MAX_T'), help='internal: one process of one variant')
    a = ap.parse_args()
    if a.one:
        return one(a.one[0], *(int(v) for v in a.one[1:]))
    sources = ('enumerated', 'sampled') + (('enumerated_parent',) if a.parent_tree else ())
    variants = [(source, n, 20, max_t) for n in (300, 1024) for max_t in (a.max_t, 1) for source in sources]
    variants += [('sampled', 1024, 1024, a.max_t), ('sampled', 1024, 1024, 1)]
    runs = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v in variants:                  # alternated: a drift of the device shows in every variant alike
            cmd = [sys.executable, os.path.abspath(__file__), '--one', v[0], str(v[1]), str(v[2]), str(a.count), str(v[3])]
            env = dict(os.environ)
            env.pop('BSX_BENCH_TREE', None)
            if v[0] == 'enumerated_parent':
                env['BSX_BENCH_TREE'] = os.path.abspath(a.parent_tree)
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
            if res.returncode != 0:
                sys.exit('variant {} failed:\n{}'.format(v, res.stdout + res.stderr))
            runs[v].append(json.loads(res.stdout.splitlines()[-1]))
    out = []
    for (source, n, n_any, max_t), rs in runs.items():
        out.append({'source': source, 'n': n, 'k': 2, 'n_any': n_any, 'count': a.count, 'max_t': max_t, 'processes': len(rs),
                    'kernel_ms': [min(r['kernel_ms'] for r in rs), max(r['kernel_ms'] for r in rs)],
                    'total_ms': [min(r['total_ms'] for r in rs), max(r['total_ms'] for r in rs)],
                    'attractors': rs[-1]['attractors'], 'none': rs[-1]['none'], 'executed_steps': rs[-1]['executed_steps'],
                    'host_syncs': rs[-1]['host_syncs']})
    print(json.dumps({'protocol': 'second of two calls in a fresh process; [min, max] over the processes; variants alternated',
                      'cases': out}, indent=1))


if __name__ == '__main__':
    main()
