"""
tests/corr_ref.py, the exact integer reference of the node correlations, against the present host path
(attractor_analysis.compute_frequency_spearmanrho: numpy ranks, np.cov) where that path is sound: total frequency
T <= 2^20.  Ranks and the NaN pattern must be equal, rho within 1e-12.

At T around 2^40 the two are not compared, and test_constant_column_at_large_total shows why: np.cov centres the ranks
with a rounded float mean, so a node that is constant over the table gets a tiny non-zero variance and its pairs a
meaningless rho instead of NaN.  The reference (and the device formulation it mirrors) has exactly zero there.
"""
import random

import numpy as np
import pytest

from boolsi_amd.attractor_analysis import compute_frequency_spearmanrho, weighted_ranks

import corr_ref
from test_profile_host import attractor_sets

LENGTHS = (1, 2, 3, 7, 12, 1023)


def table_of_set(rows):
    on = np.array([np.array(states, dtype=np.uint32).sum(axis=0) for _, _, _, states in rows], np.uint32)
    return on, [length for _, length, _, _ in rows], [f for _, _, f, _ in rows]


def random_table(seed, n, m, total_bits):
    """n attractors x m nodes; lengths from LENGTHS, on-counts with many ties (a constant node, a two-valued node, one
    that is a fixed share of the length), frequencies summing to at most 2^total_bits"""
    rng = random.Random(seed)
    lengths = [rng.choice(LENGTHS) for _ in range(n)]
    on = np.zeros((n, m), np.uint32)
    for q, length in enumerate(lengths):
        for i in range(m):
            kind = i % 4
            on[q, i] = (0 if kind == 0 else length * rng.getrandbits(1) if kind == 1 else
                        length // 2 if kind == 2 and length % 2 == 0 else rng.randint(0, length))
    cap = max(1, (1 << total_bits) // n)
    freq = [rng.randint(1, cap) for _ in range(n)]
    return on, lengths, freq


def host_path(on, lengths, freq):
    obs = corr_ref.observations(on, lengths)
    f = np.array(freq)
    ranks = np.column_stack([weighted_ranks(obs[:, j], f) for j in range(obs.shape[1])])
    rho, _ = compute_frequency_spearmanrho(obs, f)
    return ranks, rho


def compare(on, lengths, freq):
    ref = corr_ref.reference(on, lengths, freq)
    assert ref['total'] <= 1 << 20
    ranks, rho = host_path(on, lengths, freq)
    assert np.array_equal(ranks, ref['ranks'])
    assert np.array_equal(np.isnan(rho), np.isnan(ref['rho']))
    both = ~np.isnan(rho)
    worst = float(np.max(np.abs(rho[both] - ref['rho'][both]))) if both.any() else 0.0
    print('T = {}: max |rho_host - rho_exact| = {:.3g}'.format(ref['total'], worst))
    assert worst <= 1e-12
    # the reference's own invariants: S symmetric, diagonal 1, the weighted mean of rank2 is T + 1 in every column
    assert all(ref['S'][a, b] == ref['S'][b, a] for a in range(on.shape[1]) for b in range(a))
    assert all(ref['rho'][a, a] == 1.0 for a in range(on.shape[1]) if ref['S'][a, a] != 0)
    f = np.array([int(x) for x in freq], object)
    assert all(int((ref['rank2'][:, i] * f).sum()) == ref['total'] * (ref['total'] + 1) for i in range(on.shape[1]))
    return ref


@pytest.mark.parametrize('name', [name for name, rows in attractor_sets() if len(rows) > 1 and sum(r[2] for r in rows) > 2])
def test_reference_agrees_with_host_path_on_the_profile_sets(name):
    compare(*table_of_set(dict(attractor_sets())[name]))


@pytest.mark.parametrize('seed,n,m,total_bits', [(1, 2, 3, 4), (2, 5, 5, 8), (3, 40, 9, 14), (4, 300, 6, 19), (5, 1000, 4, 20)])
def test_reference_agrees_with_host_path_on_random_tables(seed, n, m, total_bits):
    on, lengths, freq = random_table(seed, n, m, total_bits)
    ref = compare(on, lengths, freq)
    if n >= 40:         # not vacuous: a NaN pair (the constant node), a pair strictly between 0 and 1, ties, several lengths
        rho = ref['rho']
        assert np.isnan(rho[0]).all() and (np.abs(rho[~np.isnan(rho)]) < 1).any() and (np.abs(rho[~np.isnan(rho)]) > 0).any()
        assert len(set(lengths)) > 1 and len(set(ref['rank2'][:, 1].tolist())) < n


def test_equal_quotients_tie_and_unequal_ones_do_not():
    # 1/2 = 2/4 = 105/210 and 1/3 = 341/1023 are each one float64 (IEEE division is correctly rounded, and the
    # quotients are the same rational): they tie.  342/1023 is another number: it does not.
    col0 = np.array([[1], [2], [105], [0]], np.uint32)
    obs = corr_ref.observations(col0, [2, 4, 210, 5])
    assert obs[0, 0] == obs[1, 0] == obs[2, 0] == 0.5
    r2, total = corr_ref.exact_rank2(col0, [2, 4, 210, 5], [1, 1, 1, 1])
    assert total == 4 and r2[:, 0].tolist() == [6, 6, 6, 2]              # 2 * 1 + 3 + 1; the zero: 0 + 1 + 1
    col1 = np.array([[1], [341], [342]], np.uint32)
    obs = corr_ref.observations(col1, [3, 1023, 1023])
    assert obs[0, 0] == obs[1, 0] != obs[2, 0]
    r2, _ = corr_ref.exact_rank2(col1, [3, 1023, 1023], [1, 1, 1])
    assert r2[:, 0].tolist() == [3, 3, 6]


def test_constant_column_at_large_total():
    """5 attractors, 5 nodes, frequencies around 2^40: node 0 is constant.  Exact arithmetic: its 9 pairs (row and
    column 0) are NaN.  numpy: none is."""
    on = np.array([[1, 1, 1, 0, 0], [1, 0, 0, 0, 0], [1, 1, 1, 1, 1], [1, 1, 0, 1, 0], [3, 0, 3, 0, 2]], np.uint32)
    lengths = [1, 1, 1, 1, 3]
    freq = [1099512452319, 1099511392682, 1099511823151, 1099511790439, 1099511046869]      # 2^40 and a little
    ref = corr_ref.reference(on, lengths, freq)
    assert ref['S'][0, 0] == 0 and int(np.isnan(ref['rho']).sum()) == 9
    _, rho = host_path(on, lengths, freq)
    print('numpy NaN entries at T ~ 2^40:', int(np.isnan(rho).sum()), 'exact:', 9)
    assert int(np.isnan(rho).sum()) == 0          # the defect of the float path, and why it is no reference up here
    ok = ~np.isnan(ref['rho'])
    assert np.max(np.abs(rho[ok] - ref['rho'][ok])) <= 1e-9      # where rho exists the two still agree
