"""
Mutant screens (DESIGN.md §3 "Mutant screens") next to what a user did before them, on n300 and n1024 of
tests/sampled_cases.py: all single mutants (every node the origin does not fix, at 0 and at 1) plus the wild type, N = 2^12
samples each.

  screen      (a) the one bsx_run_screen_sampled call;
  screen_wild the same call with the wild type listed n_mutants times: the screen's kernels over as many trajectories, every
              group as long as every other (no mutant runs longer than another);
  loop        (b) per mutant bsx_set_problem_space (the node moved from the 'any' list, where it was there, to the fixed
              nodes) + bsx_run_attract_sampled: only the two engine calls are timed, not the Python that prepares the space;
  floor       (c) one bsx_run_attract_sampled call over n_mutants * N samples of the wild type: the same number of
              trajectories through the kernel the screen's was derived from.

Protocol: one warm-up pass and `repeats` measured passes of a variant in a fresh process; three processes per variant,
the variants alternated; the median over all measured passes and their [min, max] are reported for total_ms (wall time of
the engine calls) and kernel_ms (device time between the events around the launches).
--parent-tree DIR runs (b) and (c) in another build of the project (a built checkout of the parent commit), whose entry
points they are.

    python tools/bench_screen.py [--samples N] [--rounds R] [--repeats K] [--parent-tree DIR] > profiles/mutant_screen.json
"""
import argparse
import dataclasses
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (a --one child of the parent baseline imports the package of that tree instead; the cases are this tree's)
sys.path.insert(0, os.environ.get('BSX_BENCH_TREE') or ROOT)
sys.path.insert(1, os.path.join(ROOT, 'tests'))
SEED = 7


def fixed_space(space, node, value):
    """The space a user gets by listing `node` under `fixed nodes`: out of the 'any' list where it was there."""
    import numpy as np
    fixed = np.array(sorted(space.fixed.tolist() + [[node, value]]), np.uint32).reshape(-1, 2)
    any_nodes = np.array([a for a in space.any_nodes.tolist() if a != node], np.uint32)
    return dataclasses.replace(space, fixed=fixed, any_nodes=any_nodes, n_problems=1 << len(any_nodes), radices=[2] * len(any_nodes))


def one(variant, name, samples, repeats):
    import sampled_cases
    from boolsi_amd.engine import Engine
    net, space, _ = sampled_cases.compiled(name)
    free = [i for i in range(net.n_nodes) if i not in {int(v) for v, _ in space.fixed.tolist()}]
    mutants = [()] + [((v, c),) for v in free for c in (0, 1)]
    spaces = [space] + [fixed_space(space, v, c) for v in free for c in (0, 1)] if variant == 'loop' else None
    passes = []
    with Engine(0) as eng:
        eng.set_problem(net, space)
        for _ in range(repeats + 1):
            t0 = time.perf_counter()
            if variant in ('screen', 'screen_wild'):
                records, none, st = eng.screen_sampled(SEED, 0, samples, mutants if variant == 'screen' else [()] * len(mutants), cap=1 << 18)
                kernel_ms, syncs, launches, steps = st['kernel_ms'], st['host_syncs'], st['kernel_launches'], st['executed_steps']
                found = sum(len(r) for r in records)
            elif variant == 'loop':
                kernel_ms, syncs, launches, steps, found = 0.0, 0, 0, 0, 0
                for sp in spaces:
                    eng.set_space(sp)
                    r = eng.attract_sampled(SEED, 0, samples)
                    kernel_ms += r.stats['kernel_ms']; syncs += r.stats['host_syncs']; launches += r.stats['kernel_launches']
                    steps += r.stats['executed_steps']; found += len(r.table)
            else:
                r = eng.attract_sampled(SEED, 0, samples * len(mutants), cap=1 << 18)
                kernel_ms, syncs, launches, steps, found = (r.stats['kernel_ms'], r.stats['host_syncs'], r.stats['kernel_launches'],
                                                            r.stats['executed_steps'], len(r.table))
            passes.append({'total_ms': (time.perf_counter() - t0) * 1e3, 'kernel_ms': kernel_ms, 'host_syncs': syncs,
                           'kernel_launches': launches, 'executed_steps': steps, 'records': found})
    print(json.dumps({'mutants': len(mutants), 'passes': passes[1:]}))


def spread(values):
    return {'median': statistics.median(values), 'min': min(values), 'max': max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=1 << 12)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--cases', default='n300,n1024')
    ap.add_argument('--parent-tree', metavar='DIR', help='a built checkout of the parent commit: (b) and (c) run there')
    ap.add_argument('--one', nargs=4, metavar=('VARIANT', 'CASE', 'SAMPLES', 'REPEATS'), help='internal: one process of one variant')
    a = ap.parse_args()
    if a.one:
        return one(a.one[0], a.one[1], int(a.one[2]), int(a.one[3]))
    variants = [(variant, name) for name in a.cases.split(',') for variant in ('screen', 'screen_wild', 'loop', 'floor')]
    runs = {v: [] for v in variants}
    n_mutants = {}
    for _ in range(a.rounds):
        for v in variants:                  # alternated: a drift of the device shows in every variant alike
            cmd = [sys.executable, os.path.abspath(__file__), '--one', v[0], v[1], str(a.samples), str(a.repeats if v[0] != 'loop' else 1)]
            env = dict(os.environ)
            env.pop('BSX_BENCH_TREE', None)
            if v[0] in ('loop', 'floor') and a.parent_tree:
                env['BSX_BENCH_TREE'] = os.path.abspath(a.parent_tree)
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, env=env)
            if res.returncode != 0:
                sys.exit('variant {} failed:\n{}'.format(v, res.stdout + res.stderr))
            got = json.loads(res.stdout.splitlines()[-1])
            n_mutants[v[1]] = got['mutants']
            runs[v].extend(got['passes'])
    cases = []
    for (variant, name), ps in runs.items():
        trajectories = n_mutants[name] * a.samples
        total, kernel = spread([p['total_ms'] for p in ps]), spread([p['kernel_ms'] for p in ps])
        cases.append({'variant': variant, 'case': name, 'mutants': n_mutants[name], 'samples': a.samples, 'trajectories': trajectories,
                      'build': 'parent' if variant in ('loop', 'floor') and a.parent_tree else 'this', 'passes': len(ps),
                      'total_ms': total, 'kernel_ms': kernel,
                      'kernel_ns_per_trajectory': {k: 1e6 * v / trajectories for k, v in kernel.items()},
                      'host_syncs': ps[-1]['host_syncs'], 'kernel_launches': ps[-1]['kernel_launches'],
                      'executed_steps': ps[-1]['executed_steps'], 'records': ps[-1]['records']})
    by = {(c['variant'], c['case']): c for c in cases}
    ratios = [{'case': name,
               'loop_over_screen_total': by[('loop', name)]['total_ms']['median'] / by[('screen', name)]['total_ms']['median'],
               'screen_over_floor_kernel_per_trajectory': by[('screen', name)]['kernel_ms']['median'] / by[('floor', name)]['kernel_ms']['median'],
               'screen_wild_over_floor_kernel_per_trajectory': by[('screen_wild', name)]['kernel_ms']['median'] / by[('floor', name)]['kernel_ms']['median']}
              for name in a.cases.split(',')]
    print(json.dumps({'protocol': 'one warm-up pass, then measured passes in a fresh process; median and [min, max] over all measured '
                                  'passes of all processes; variants alternated (loop: one measured pass per process)',
                      'cases': cases, 'ratios': ratios}, indent=1))


if __name__ == '__main__':
    main()
