"""
The cube cascade at production size against an independent exact reference: product networks (tests/product_family.py)
whose attract table over any index range follows from their components' functional graphs by integer combinatorics
(tests/product_ref.py, itself held to the CPU oracle in tests/test_product_ref.py).  At n = 64: blocks of 2^48, 2^52 and 2^56
problems, ragged ranges, forced sub-blocks and depths, a length cap, and a time cap inside the transients on two of the four
members; at n = 32 and 48 the same scaled down, whole spaces included; at n = 96 blocks up to 2^63 and 2^64 consecutive
problems across the 64-digit boundary.  What is not listed and why (no n = 64 block beyond 2^56, capped calls that do not
collapse) is in product_family.py's ladder notes.  Keys, lengths, counts, sums of transients and of their squares,
no-attractor counts and the reference step count, all by integer equality.  The engine sees one ordinary network; it
knows nothing of the factors.

And the north star itself: each attractor's exact mean transient over all 2^64 initial states against the mean of
2^16 problems walked by the oracle.
"""
import os
from math import sqrt

import pytest

import product_family as F
from boolsi_amd import synth
from boolsi_amd.attract import record_ints
from boolsi_amd.compile import compile_problem
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text

pytestmark = pytest.mark.gpu
KNOBS = ('BSX_CUBES', 'BSX_CUBE_DEPTH', 'BSX_CUBE_NEAR_CAP', 'BSX_CUBE_LOWER', 'BSX_CUBE_LEAF', 'BSX_SPIN_WAIT', 'BSX_CUBE_SPLIT', 'BSX_CUBE_STREAMS')
CASES = [(m.name, i) for m in F.members() for i in range(len(m.calls))]


def case_id(case):
    name, i = case
    c = {m.name: m for m in F.members()}[name].calls[i]
    size = '2p{}'.format(c.count.bit_length() - 1) + ('' if c.count & (c.count - 1) == 0 else '_ragged')
    extra = ''.join('_{}{}'.format(k[4:].lower(), v) for k, v in c.env)
    extra += '' if c.max_t == F.INF else '_cap{}'.format(c.max_t)
    extra += '' if c.max_len == F.INF else '_len{}'.format(c.max_len)
    return '{}-{}-{}{}'.format(name, i, size, extra)


@pytest.fixture(scope='module')
def eng():
    from boolsi_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope='module')
def compiled():
    """name -> (member, net, space); the components' functional graphs are computed once per member (Member.components)."""
    out = {}
    for m in F.members():
        net, space = compile_problem(parse_input_text(m.yaml(), F.INF, Mode.ATTRACT))
        out[m.name] = (m, net, space)
    return out


@pytest.fixture()
def knobs():
    yield
    for k in KNOBS:
        os.environ.pop(k, None)


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_product_network_table_equals_the_exact_reference(eng, compiled, knobs, case):
    name, i = case
    m, net, space = compiled[name]
    c = m.calls[i]
    want_table, want_none, want_steps = m.table(c)
    for k in KNOBS:
        os.environ.pop(k, None)
    eng.set_problem(net, space)                                             # fresh journal, no calibration
    eng.attract2(c.first, min(c.count, 1 << 20), c.max_t, c.max_len)        # discovery
    os.environ.update(dict(c.env))
    got = eng.attract2(c.first, c.count, c.max_t, c.max_len)
    rows = sorted(record_ints(a) for a in got.table)
    assert rows == sorted((key,) + tuple(e) for key, e in want_table.items())
    assert got.n_no_attractor == want_none
    assert got.stats['state_steps'] == want_steps and got.stats['problems'] == c.count
    if c.count >= 1 << 48 and c.count & (c.count - 1) == 0 and c.first % c.count == 0:
        # the cube cascade did it, not the ladder of fall-backs underneath
        assert got.stats['dominant_launches'] >= 1 and got.stats['executed_steps'] < c.count >> 8


def test_north_star_mean_transients_against_the_oracle_sample(eng):
    """One attract2 over all 2^64 initial states: each attractor's exact mean transient sum_l / count lies within
    6 s / sqrt(n_a) of the mean over the n_a sampled problems that the oracle walked into it, s their own standard deviation."""
    sample, lost = F.north_star_sample()
    assert lost == 0
    net, space = compile_problem(parse_input_text(synth.north_star_yaml(), 4096, Mode.ATTRACT))
    eng.set_problem(net, space)
    eng.attract(0, 1 << 30, 4096)
    got = eng.attract2(0, 1 << 64, 4096)
    table = {r[0]: r for r in (record_ints(a) for a in got.table)}
    assert set(table) == set(F.NORTH_STAR) == set(sample)
    for key, (length, n_a, s1, s2) in sample.items():
        _, glen, count, sum_l, _ = table[key]
        assert (glen, count) == F.NORTH_STAR[key] and glen == length
        mean = s1 / n_a
        s = sqrt((s2 - s1 * s1 / n_a) / (n_a - 1))
        print('north star {:#x}: exact mean {:.4f}, sampled {:.4f} +- {:.4f} ({} samples)'.format(key, sum_l / count, mean, s / sqrt(n_a), n_a))
        assert abs(sum_l / count - mean) <= 6 * s / sqrt(n_a)
