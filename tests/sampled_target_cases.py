"""
TEST INFRASTRUCTURE -- target substates and reference results of the sampled target and simulate tests
(tests/test_sampled_target_ref.py on the CPU; tests/test_gpu_sampled_target.py, tests/test_gpu_sampled_simulate.py and
tests/test_gpu_sampled_target_cli.py on the GPU).  The networks and spaces are those of sampled_cases.py; the reference of
a sampled call is sample_ref.sample_indices fed to WideRef.target / .simulate / .trajectories and nothing else.

A range is 32 L + 37 samples from FIRST with SEED (L: columns per workgroup, sampled_cases.L_OF): unaligned, with a ragged
second group.  The substates were found on the CPU so that expect_target's assertions hold.

state_steps of a target call is the sum of the times at which the searches ended.  A hit ends at its time, a search that
runs into the cap at the cap.  A miss whose cycle closes ends where the kernel's detector sees that, which is later than the
reference's first repeated state: Brent's detector keeps a checkpoint s(c_i), c_i = T_max + 2^i - 1 with T_max the largest
T_p of the trajectory's group, for 2^i steps, and sees the cycle at the first t = c_i + lambda with c_i on the cycle
(c_i >= T_p + mu) and lambda <= 2^i.  brent_stop below restates that; mu and lambda come from the reference.
"""
import functools

import sample_ref
from sampled_cases import FIRST, L_OF, SEED, compiled

INF = None
GENEROUS = 400

# name -> (target nodes, target substate code, splitting cap)
TARGETS = {
    'n257': ([114, 230, 256], (1 << 114) | (1 << 230), 2),
    'n577': ([5, 100, 416, 537, 576], (1 << 5) | (1 << 100) | (1 << 576), 2),
    'n600_9_inputs': ([55, 224], 1 << 55, 7),
    'n1024': ([5, 100, 640, 984, 1023], 1 << 5, 5),
    'n700_variations': ([2, 40, 300, 640, 650], 0, 12),
    'n64': ([1, 2, 3], 1 << 3, 5),
    'n300': ([241, 246, 299], 1 << 241, 14),
    'example2': ([0, 1], 1 << 1, 0),
}
# cases small enough that only "a hit and a miss" can be asked of them (example2 has eight states)
RELAXED = {'example2'}


def count_of(name):
    return 32 * L_OF[name] + 37


@functools.lru_cache(maxsize=None)
def indices(name, first, count, seed=SEED):
    return sample_ref.sample_indices(compiled(name)[1], seed, range(first, first + count))


def brent_stop(t_max, on_cycle_at, lam):
    """The time at which Brent's detector with checkpoints T_max + 2^i - 1 sees a cycle of length lam that the trajectory
    is on from t = on_cycle_at."""
    i = 0
    while True:
        c = t_max + (1 << i) - 1
        if c >= on_cycle_at and lam <= (1 << i):
            return c + lam
        i += 1


@functools.lru_cache(maxsize=None)
def target_ends(name, first, count, max_t=INF, seed=SEED, group=None):
    """Per sample of [first, first + count): (reached, t at which its search ends in a launch over exactly that range).
    group: samples per group (default 32 L of the case)."""
    net, space, ref = compiled(name)
    nodes, code, _ = TARGETS[name]
    idx = indices(name, first, count, seed)
    import numpy as np
    values = np.array([(code >> i) & 1 for i in sorted(nodes)], np.uint8)
    free = ref.search(idx, None, (np.array(sorted(nodes), np.int64), values))
    G = group or 32 * L_OF[name]
    out = []
    for q, r in enumerate(free):
        t_max = max(x['tp'] for x in free[q - q % G:q - q % G + G])
        if r['reached']:
            end = r['t']
            hit = max_t is None or end <= max_t
            out.append((hit, end if hit else max_t))
        else:
            assert r['found'], 'a miss at max_t = inf is a closed cycle'
            end = brent_stop(t_max, r['tp'] + r['mu'], r['lam'])
            out.append((False, end if max_t is None or end <= max_t else max_t))
    return out


def hits_of(ends):
    return [(q, t) for q, (reached, t) in enumerate(ends) if reached]


def histogram(hits, bins=8):
    return [sum(1 for _, t in hits if t == b) for b in range(bins - 1)] + [sum(1 for _, t in hits if t >= bins - 1)]


@functools.lru_cache(maxsize=None)
def expect_target(name):
    """-> {cap: (hits [(offset, t)], state_steps)} for the splitting cap, GENEROUS and INF, with the assertions that the
    case is not vacuous, from the reference alone."""
    net, space, ref = compiled(name)
    nodes, code, split = TARGETS[name]
    count, G = count_of(name), 32 * L_OF[name]
    out = {}
    for cap in (split, GENEROUS, INF):
        ends = target_ends(name, FIRST, count, cap)
        out[cap] = (hits_of(ends), sum(t for _, t in ends))
    # the reference's own target search agrees with the ends above on what it defines: who hits, and when
    res = ref.target(indices(name, FIRST, count), None, nodes, code)
    assert [(q, t) for q, (reached, t) in enumerate(res) if reached] == out[INF][0]
    hits = out[INF][0]
    assert 0 < len(hits) < count, 'no hit or no miss'
    assert 0 < len(out[split][0]) < len(hits), 'the splitting cap does not split'
    assert out[GENEROUS][0] == hits, 'the generous cap cuts a hit off'
    if name not in RELAXED:
        tps = [ref.problem(i).tp for i in indices(name, FIRST, count)]
        assert len({t for _, t in hits}) >= 3, 'fewer than three first-hit times'
        assert max(t for _, t in hits) > max(tps), 'no hit later than the largest T_p'
        assert any(q < G for q, _ in hits) and any(q >= G for q, _ in hits), 'a group without a hit'
    return out
