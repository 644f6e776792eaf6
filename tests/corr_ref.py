"""
Exact reference of the node correlations (bsx_run_node_correlations, attractor_analysis.find_node_correlations), in
Python integers.

Input: on_counts (n, n_nodes), lengths (n), frequencies (n, Python ints).  An observation is the float64 quotient
on_count / length -- the same IEEE division the host path and the device make; two attractors tie in a column exactly
when those doubles are equal.  From there on nothing is rounded:
    rank2[q][i] = 2 W_less + W_equal + 1            twice the average rank
    d2          = rank2 - (T + 1)                   twice the centred rank, T the total frequency
    S[a][b]     = sum_q f_q d2[q][a] d2[q][b]
rho = S_ab / sqrt(S_aa S_bb) is formed with 60 decimal digits and rounded to float64 once; it is NaN iff S_aa S_bb == 0.
"""
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np


def observations(on_counts, lengths):
    return np.asarray(on_counts, np.float64) / np.asarray(lengths, np.float64)[:, None]


def exact_rank2(on_counts, lengths, frequencies):
    """-> (rank2 as an (n, n_nodes) object array of ints, T)"""
    obs = observations(on_counts, lengths)
    n, m = obs.shape
    f = [int(x) for x in frequencies]
    total = sum(f)
    rank2 = np.zeros((n, m), object)
    for i in range(m):
        weight = {}
        for q, v in enumerate(obs[:, i].tolist()):
            weight[v] = weight.get(v, 0) + f[q]
        less, r2 = 0, {}
        for v in sorted(weight):
            r2[v] = 2 * less + weight[v] + 1
            less += weight[v]
        rank2[:, i] = [r2[v] for v in obs[:, i].tolist()]
    return rank2, total


def exact_s(rank2, total, frequencies):
    """S as an (n_nodes, n_nodes) object array of Python ints"""
    f = np.array([int(x) for x in frequencies], object)
    d2 = rank2 - (total + 1)
    biggest = max(abs(int(x)) for x in d2.ravel()) if d2.size else 0
    if total * biggest * biggest < 1 << 62:                 # every partial sum fits int64: an exact integer matmul
        d = d2.astype(np.int64)
        return (d.T @ (d * f.astype(np.int64)[:, None])).astype(object)
    return d2.T.dot(d2 * f[:, None])


def exact_rho(S):
    """float64 rho from the exact S: 60-digit arithmetic, NaN iff S_aa S_bb == 0"""
    m = S.shape[0]
    rho = np.full((m, m), np.nan)
    with localcontext() as ctx:
        ctx.prec = 60
        root = [Decimal(int(S[a, a])).sqrt() for a in range(m)]
        for a in range(m):
            if S[a, a] == 0:
                continue
            for b in range(a, m):
                if S[b, b] != 0:
                    rho[a, b] = rho[b, a] = float(Decimal(int(S[a, b])) / (root[a] * root[b]))
    return rho


def reference(on_counts, lengths, frequencies):
    """-> dict(rank2, ranks (float64, rank2 / 2 rounded once), total, S (ints), rho (float64))"""
    rank2, total = exact_rank2(on_counts, lengths, frequencies)
    S = exact_s(rank2, total, frequencies)
    ranks = np.array([[float(Fraction(int(x), 2)) for x in row] for row in rank2], np.float64).reshape(rank2.shape)
    return {'rank2': rank2, 'ranks': ranks, 'total': total, 'S': S, 'rho': exact_rho(S)}


def s_errors_beyond_bound(S_dev, S, n):
    """Entries with |S_dev - S| > (n + 16) 2^-52 sqrt(S_aa S_bb), decided in integers: the standard bound of a sum of n
    rounded products with Cauchy-Schwarz, valid for any order of summation; the 16 covers the roundings of the operands."""
    m = S.shape[0]
    close = S_dev == S.astype(np.float64)           # the correctly rounded value is within the bound (|S_ab| <= sqrt(S_aa S_bb))
    bad = []
    for a, b in np.argwhere(~close).tolist():
        if not np.isfinite(S_dev[a, b]):
            bad.append((a, b))
            continue
        err = Fraction(float(S_dev[a, b])) - int(S[a, b])
        if err * err * (1 << 104) > (n + 16) ** 2 * int(S[a, a]) * int(S[b, b]):
            bad.append((a, b))
    assert m == S_dev.shape[0]
    return bad


def rho_of_s(S_dev):
    """what the host forms from the device's matrix (attractor_analysis.correlation_statistics, without the p-values)"""
    var = S_dev.diagonal()
    with np.errstate(invalid='ignore', divide='ignore'):
        return S_dev / np.sqrt(np.multiply.outer(var, var))
