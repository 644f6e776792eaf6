"""
TEST INFRASTRUCTURE -- the node-influence definition of include/bsx.h (bsx_run_influence_sampled) restated on sample_ref.py
and damage_ref.step (the rules, then the origin's fixed nodes).  Nothing under boolsi_amd/ imports it.

    x(0) = sample j's state, y(0) = x(0) with node sources[s] inverted; D_j(t) = x(t) ^ y(t), t = 1 .. T
    influence[s][t - 1][i] = samples with bit i of D_j(t) set;  n_merged[s][t - 1] = samples with D_j(t) == 0
"""
import numpy as np

import damage_ref


def states(ref, seed, samples):
    """-> uint8[count, n]: x(0) of the listed samples (damage_ref.pairs without a flip)."""
    return damage_ref.pairs(ref, seed, samples, 0)[0]


def counts(ref, seed, first, count, sources, T):
    """-> (influence int64[n_sources, T, n], n_merged int64[n_sources, T]) over samples first .. first + count - 1."""
    X = [states(ref, seed, range(first, first + count))]
    for _ in range(T):
        X.append(damage_ref.step(ref, X[-1]))
    influence = np.zeros((len(sources), T, ref.n), np.int64)
    merged = np.zeros((len(sources), T), np.int64)
    for s, v in enumerate(sources):
        Y = X[0].copy()
        Y[:, v] ^= 1
        for t in range(1, T + 1):
            Y = damage_ref.step(ref, Y)
            D = X[t] ^ Y
            influence[s, t - 1] = D.sum(axis=0)
            merged[s, t - 1] = count - int(D.any(axis=1).sum())
    return influence, merged
