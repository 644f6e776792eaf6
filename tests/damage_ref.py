"""
TEST INFRASTRUCTURE -- the damage-spreading definition of include/bsx.h (bsx_run_damage_sampled) restated in Python ints
on sample_ref.py, stepping with WideRef.rules under the origin's fixed nodes.  Nothing under boolsi_amd/ imports it.

    D(j, i) = mix(kb(j >> 6) + G * (n_any + 65 + 64 i + (j & 63)))
    p       = (D(j, i) * (n_free - i)) >> 64;  for every position c chosen earlier, ascending: if p >= c then p += 1

y(0) = x(0) with free[p] inverted for the h chosen positions; d(t) = popcount(x(t) ^ y(t)).
"""
import numpy as np

import sample_ref


def positions(seed, j, n_any, n_free, h):
    """The h chosen positions of sample j, in the order they are chosen, by the definition's own loop."""
    kb, lane = sample_ref.block_key(seed, j >> 6), j & 63
    chosen = []
    for i in range(h):
        p = (sample_ref.mix(kb + sample_ref.G * (n_any + 65 + 64 * i + lane)) * (n_free - i)) >> 64
        for c in sorted(chosen):
            if p >= c:
                p += 1
        chosen.append(p)
    return chosen


def free_nodes(ref):
    fixed = {node for node, _ in ref.space.fixed.tolist()}
    return [i for i in range(ref.n) if i not in fixed]


def pairs(ref, seed, samples, h):
    """-> (X, Y) uint8[count, n]: x(0) and y(0) of the listed samples."""
    sp = ref.space
    n_any = len(sp.any_nodes)
    assert not len(sp.fixed_var) and not len(sp.pert_var) and not len(sp.sched), 'variations or a schedule'
    X = np.array([ref.problem(i).init for i in sample_ref.sample_indices(sp, seed, samples)], np.uint8).reshape(len(samples), ref.n)
    free = free_nodes(ref)
    Y = X.copy()
    for q, j in enumerate(samples):
        for p in positions(seed, int(j), n_any, len(free), h):
            Y[q, free[p]] ^= 1
    return X, Y


def step(ref, S):
    """F: the rules, then the origin's fixed nodes."""
    N = ref.rules(S)
    for node, value in ref.space.fixed.tolist():
        N[:, node] = value
    return N


def distances(ref, seed, first, count, h, T):
    """-> int64[T + 1, count]: d_j(t) of samples first .. first + count - 1."""
    X, Y = pairs(ref, seed, range(first, first + count), h)
    out = np.zeros((T + 1, count), np.int64)
    for t in range(T + 1):
        if t:
            X, Y = step(ref, X), step(ref, Y)
        out[t] = (X ^ Y).sum(axis=1)
    return out


def sums(d, n):
    """d int64[T + 1, count] -> (sum_d, sum_d2, n_merged, hist) as lists of Python ints (hist: [T + 1][n + 1])."""
    sum_d = [int(row.sum()) for row in d]
    sum_d2 = [sum(int(v) * int(v) for v in row) for row in d]
    merged = [int((row == 0).sum()) for row in d]
    hist = [np.bincount(row, minlength=n + 1).tolist() for row in d]
    return sum_d, sum_d2, merged, hist
