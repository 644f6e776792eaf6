"""
TEST INFRASTRUCTURE -- exact attract tables of *product networks* over any index range of a space of up to 2^128
problems, without walking a trajectory of the product.

A product network is a set of components, node sets that only read each other.  Every component is small enough
(m <= 22 nodes) to have its whole functional graph in memory: successor, cycles, and per state the transient mu and a
phase phi on its cycle.  The product's table then follows by integer combinatorics:

  * the joint state at time t >= max(mu_c) is (cycle_c[(phi_c + t) mod lambda_c])_c, so the joint transient is
    max(mu_c), the joint cycle length lcm(lambda_c), and the joint cycle is the orbit of the phase tuple under +1
    (a pair of cycles splits into gcd-many joint cycles by phase difference);
  * an aligned block of 2^a consecutive problems is a sub-cube of every component (some initial bits fixed, the rest
    free), the components' sub-cubes are independent, so #(joint mu <= m, joint cycle state at time 0 = g) is the
    product of the components' own cumulative counts;
  * any range [lo, hi) is at most 2 x 128 aligned blocks (binary decomposition).

Semantics (oracle/bsx_oracle.c: simulate_until + solve_all_states + orc_run_attract, no perturbations, T_p = 0): the
walk stops at the first repeated state, t = mu + lambda, or at max_t; found iff mu + lambda <= max_t; a found problem
with lambda > max_len counts as no attractor; trajectory_l = mu; state_steps = min(mu + lambda, max_t) per problem;
key = the smallest state code on the cycle (node i = bit i).

numpy and Python ints only; neither the engine nor the oracle is imported here.
"""
from math import gcd

import numpy as np

INF = float('inf')


def component(preds, masks):
    """preds[i]: local indices of node i's inputs, masks[i]: its truth table, bit idx = output when input j has state
    (idx >> j) & 1 (the order synth.rule_text documents) -> the functional graph of the 2^m states:
        m, succ[s], cycles (list of ordered state lists), att[s], mu[s], phi[s] with
        state of s at any time t >= mu[s] == cycles[att[s]][(phi[s] + t) % len(cycles[att[s]])],
        gidx[s] = number of the cycle state cycles[att[s]][phi[s]] among all cycle states (cycle after cycle),
        g_att[g], g_len[g], g_state[g] per cycle state number."""
    m = len(preds)
    assert 1 <= m <= 22 and len(masks) == m
    size = 1 << m
    states = np.arange(size, dtype=np.uint32)
    succ = np.zeros(size, np.uint32)
    for i in range(m):
        idx = np.zeros(size, np.uint32)
        for j, p in enumerate(preds[i]):
            idx |= ((states >> np.uint32(p)) & np.uint32(1)) << np.uint32(j)
        table = np.array([(masks[i] >> r) & 1 for r in range(1 << len(preds[i]))], np.uint32)
        succ |= table[idx] << np.uint32(i)
    # cycle states = image of f^(2^m): m doublings of the successor array
    g = succ.copy()
    for _ in range(m):
        g = g[g]
    on_cycle = np.zeros(size, bool)
    on_cycle[g] = True
    att = np.full(size, -1, np.int64)
    mu = np.full(size, -1, np.int64)
    phi = np.zeros(size, np.int64)
    cycles = []
    for s in np.flatnonzero(on_cycle).tolist():
        if att[s] >= 0:
            continue
        cyc, x = [], s
        while att[x] < 0:
            att[x], mu[x], phi[x] = len(cycles), 0, len(cyc)
            cyc.append(x)
            x = int(succ[x])
        assert x == s
        cycles.append(cyc)
    lens = np.array([len(c) for c in cycles], np.int64)
    # transient states, level by level: s at time t is f(s) at time t - 1
    rem = np.flatnonzero(mu < 0)
    while rem.size:
        nxt = succ[rem]
        hit = mu[nxt] >= 0
        done, to = rem[hit], nxt[hit]
        assert done.size
        att[done] = att[to]
        mu[done] = mu[to] + 1
        phi[done] = (phi[to] - 1) % lens[att[to]]
        rem = rem[~hit]
    offs = np.concatenate([[0], np.cumsum(lens)])
    return dict(m=m, succ=succ, cycles=cycles, att=att, mu=mu, phi=phi, gidx=offs[att] + phi,
                g_att=[a for a, c in enumerate(cycles) for _ in c], g_len=[len(c) for c in cycles for _ in c],
                g_state=[s for c in cycles for s in c], max_mu=int(mu.max()), _hist={})


def _sub_cube_hist(comp, free_bits, fixed):
    """Over the component states fixed | (any value of the free bits): cum[g][m] = states whose cycle state at time 0
    is number g and whose mu <= m, as lists of Python ints; rows of states that do not occur are None."""
    key = (tuple(free_bits), fixed)
    got = comp['_hist'].get(key)
    if got is not None:
        return got
    if len(free_bits) == comp['m']:
        gi, mu = comp['gidx'], comp['mu']
    else:
        sub = np.array([fixed], np.int64)
        for b in free_bits:
            sub = np.concatenate([sub, sub | (1 << b)])
        gi, mu = comp['gidx'][sub], comp['mu'][sub]
    width = comp['max_mu'] + 1
    n_g = len(comp['g_att'])
    hist = np.bincount(gi * width + mu, minlength=n_g * width).reshape(n_g, width)
    cum = np.cumsum(hist, axis=1)
    out = [row.tolist() if row[-1] else None for row in cum]
    if len(comp['_hist']) < 4096:
        comp['_hist'][key] = out
    return out


def blocks_of(lo, hi):
    """[lo, hi) as aligned power-of-two blocks (base, log2 size), ascending."""
    out = []
    while lo < hi:
        a = (lo & -lo).bit_length() - 1 if lo else hi.bit_length()
        while (1 << a) > hi - lo:
            a -= 1
        out.append((lo, a))
        lo += 1 << a
    return out


def placed_code(state, nodes):
    code = 0
    for j, node in enumerate(nodes):
        code |= ((state >> j) & 1) << node
    return code


def joint_cycles(components, placement):
    """Every tuple of component cycle states is a joint cycle state.  -> (shape, owner, cycles): owner[flat tuple index]
    = joint cycle number, cycles[q] = (key, length): the smallest placed state code on the orbit and lcm of the lengths."""
    shape = [len(c['g_att']) for c in components]
    total = 1
    for s in shape:
        total *= s
    codes = [[placed_code(s, placement[c]) for s in comp['g_state']] for c, comp in enumerate(components)]
    firsts = []                         # number of a cycle's first state, per component cycle state
    for comp in components:
        at, f = 0, []
        for cyc in comp['cycles']:
            f += [at] * len(cyc)
            at += len(cyc)
        firsts.append(f)
    owner = [-1] * total
    cycles = []

    def flat(t):
        v = 0
        for g, s in zip(t, shape):
            v = v * s + g
        return v

    def tuples(c):
        if c == len(shape):
            yield ()
            return
        for g in range(shape[c]):
            for rest in tuples(c + 1):
                yield (g,) + rest

    for t in tuples(0):
        if owner[flat(t)] >= 0:
            continue
        length, key, x = 0, None, t
        while owner[flat(x)] < 0:
            owner[flat(x)] = len(cycles)
            code = 0
            for c, g in enumerate(x):
                code |= codes[c][g]
            key = code if key is None else min(key, code)
            length += 1
            x = tuple(firsts[c][g] + (g - firsts[c][g] + 1) % components[c]['g_len'][g] for c, g in enumerate(x))
        assert x == t
        lcm = 1
        for c, g in enumerate(t):
            lam = components[c]['g_len'][g]
            lcm = lcm * lam // gcd(lcm, lam)
        assert lcm == length
        cycles.append((key, length))
    return shape, owner, cycles


def product_table(components, placement, lo, hi, max_t=INF, max_len=INF):
    """The attract result over the problems [lo, hi) of the product network whose component c has its bit j at node
    (= initial-state digit) placement[c][j] -> ({key: (length, count, sum_l, sum_l2)}, n_no_attractor, state_steps)."""
    n = sum(len(p) for p in placement)
    assert sorted(x for p in placement for x in p) == list(range(n))
    assert all(len(p) == c['m'] for p, c in zip(placement, components))
    assert 0 <= lo <= hi <= 1 << n
    shape, owner, cycles = joint_cycles(components, placement)
    width = max(c['max_mu'] for c in components) + 1
    # dist[q][m] = problems of the range on joint cycle q with joint transient m
    dist = [[0] * width for _ in cycles]
    for base, a in blocks_of(lo, hi):
        cums = []
        for c, comp in enumerate(components):
            free = [j for j, node in enumerate(placement[c]) if node < a]
            fixed = 0
            for j, node in enumerate(placement[c]):
                if node >= a:
                    fixed |= ((base >> node) & 1) << j
            rows = _sub_cube_hist(comp, free, fixed)
            cums.append([(g, r + [r[-1]] * (width - len(r))) for g, r in enumerate(rows) if r is not None])

        def walk(c, flat, cum):
            if c == len(cums):
                d = dist[owner[flat]]
                prev = 0
                for m in range(width):
                    d[m] += cum[m] - prev
                    prev = cum[m]
                return
            for g, row in cums[c]:
                walk(c + 1, flat * shape[c] + g, row if cum is None else [x * y for x, y in zip(cum, row)])

        walk(0, 0, None)
    table, none, steps = {}, 0, 0
    for (key, lam), d in zip(cycles, dist):
        count = s1 = s2 = 0
        for m, k in enumerate(d):
            if not k:
                continue
            if m + lam <= max_t:
                steps += (m + lam) * k
                if lam <= max_len:
                    count, s1, s2 = count + k, s1 + m * k, s2 + m * m * k
                else:
                    none += k
            else:
                steps += max_t * k
                none += k
        if count:
            table[key] = (lam, count, s1, s2)
    return table, none, steps
