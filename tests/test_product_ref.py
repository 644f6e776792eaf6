"""
tests/product_ref.py and tests/product_family.py proven on the CPU (no GPU):

  * product_table equals the CPU oracle (Oracle.attract, aggregated) to the last digit on products small enough to
    enumerate -- two and three components, contiguous and scattered placements, whole spaces, aligned blocks, ragged
    ranges, time caps from 1 through values inside and beyond the transients, length caps 1 and 2;
  * every family member fits the cycle mirror, the family shows gcd splitting, a proper lcm, a transient of 20 or more
    and blocks whose largest transient comes from different components; every listed call adds up to its range;
  * the north star's two basins, pinned as exact integers elsewhere, against 2^16 problems sampled through the oracle.
"""
import os
import random
from math import gcd, sqrt

import pytest

import product_family as F
import product_ref as R
from boolsi_amd.attract import merge_tables
from boolsi_amd.compile import compile_problem
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text

CORES = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
INF = float('inf')


def scattered(sizes, seed):
    nodes = list(range(sum(sizes)))
    random.Random(seed).shuffle(nodes)
    out, at = [], 0
    for m in sizes:
        out.append(nodes[at:at + m])
        at += m
    return out


SMALL = {
    # (m, K, seed): cycle lengths of the component, largest mu
    'two_contiguous': ([(8, 2, 1), (9, 2, 3)], F.contiguous([8, 9])),                    # [2, 4] 8; [4, 4, 12, 12] 7: gcd 2 and 4
    'two_scattered': ([(10, 2, 3), (7, 2, 28)], scattered([10, 7], 1)),                  # [1, 1, 5] 15; [4, 6] 5: lcm 20, 30
    'three_contiguous': ([(6, 2, 27), (7, 2, 14), (6, 2, 14)], F.contiguous([6, 7, 6])),  # [1, 2, 3]; [2, 2, 3, 3]; [2, 2]
    'three_scattered_k3': ([(6, 2, 9), (8, 3, 4), (6, 2, 31)], scattered([6, 8, 6], 2)),  # [1, 2, 2]; K = 3 [1, 2, 5] 22; [1, 5]
    'three_interleaved': ([(6, 2, 7), (6, 2, 17), (6, 2, 12)], F.interleaved(18, 3)),    # [1, 8]; [1, 1, 2]; [1, 3]
}


def oracle_result(orc, first, count, max_t, max_len):
    _, table, none, steps = orc.attract(first, count, max_t, max_len, per_problem=False, n_threads=min(CORES, 16))
    return {k: tuple(v) for k, v in merge_tables([table]).items()}, none, steps


@pytest.mark.parametrize('name', sorted(SMALL))
def test_product_table_equals_the_oracle(name):
    from oracle.cpu_oracle import Oracle
    parts, placement = SMALL[name]
    member = F.Member(name, tuple(parts), placement, [], 0)
    n, comps = member.n, member.components()
    net, space = compile_problem(parse_input_text(member.yaml(), INF, Mode.ATTRACT))
    assert space.any_nodes.tolist() == list(range(n))
    orc = Oracle(net, space)
    total = 1 << n
    deep = member.largest_mu_plus_lambda()
    rng = random.Random(n)
    ranges = [(0, total), (0, total >> 3), (5 << (n - 3), total >> 3), (total - (1 << (n - 6)), 1 << (n - 6)), (3 << 7, 1 << 7),
              (12345, (total >> 1) + 4321), (total - 99999, 99999), (1, 1), (total - 1, 1), (777, 2)]
    ranges += [(lo, rng.randrange(1, min(total - lo, 1 << 14) + 1)) for lo in (rng.randrange(total) for _ in range(6))]
    for first, count in ranges:
        whole = first == 0 and count == total
        caps = [(INF, INF)]
        if whole or count <= 1 << (n - 3):
            caps += [(1, INF), (2, INF), (3, INF), (deep // 2, INF), (deep - 1, INF), (deep, INF), (deep + 5, INF), (INF, 1), (INF, 2),
                     (deep // 2, 2), (4, 1)]
        for max_t, max_len in caps:
            want = oracle_result(orc, first, count, max_t, max_len)
            got = R.product_table(comps, placement, first, first + count, max_t, max_len)
            assert got == want, (name, first, count, max_t, max_len)
            assert sum(e[1] for e in got[0].values()) + got[1] == count
            if whole and max_t == INF and max_len == INF:             # (not a product of fixed points)
                assert len(got[0]) >= 3 and max(e[0] for e in got[0].values()) >= 4 and max(c['max_mu'] for c in comps) >= 5


def test_blocks_of_cover_the_range_with_aligned_blocks():
    rng = random.Random(5)
    for _ in range(200):
        lo = rng.getrandbits(rng.randrange(1, 129))
        hi = lo + rng.getrandbits(rng.randrange(1, 129))
        hi = min(hi, 1 << 128)
        at = lo
        blocks = R.blocks_of(lo, hi)
        for base, a in blocks:
            assert base == at and base % (1 << a) == 0
            at += 1 << a
        assert at == max(lo, hi) and len(blocks) <= 2 * 128
    assert R.blocks_of(0, 1 << 64) == [(0, 64)]


# ---- the family ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def family():
    return {m.name: m for m in F.members()}


def joint(member):
    return R.joint_cycles(member.components(), member.placement)[2]


def test_family_selection(family):
    assert {m.n for m in family.values()} == {32, 48, 64, 96}
    splits = proper = 0
    for m in family.values():
        comps, cycles = m.components(), joint(m)
        assert len(cycles) <= 64 and max(length for _, length in cycles) <= 64, m.name
        assert sum(length for _, length in cycles) <= F.MIRROR_STATES[m.n], m.name
        lens = [sorted({len(c) for c in comp['cycles']}) for comp in comps]
        splits += any(gcd(a, b) > 1 for i, la in enumerate(lens) for lb in lens[i + 1:] for a in la for b in lb)
        proper += max(length for _, length in cycles) > max(max(la) for la in lens)
        assert m.largest_mu_plus_lambda() // 2 <= F.CAP[m.name] < m.largest_mu_plus_lambda()
        assert sorted(x for p in m.placement for x in p) == list(range(m.n))
    assert splits >= 1 and proper >= 1
    assert max(c['max_mu'] for m in family.values() for c in m.components()) >= 20
    figures = {name: (len(joint(m)), sum(length for _, length in joint(m)), sorted(length for _, length in joint(m))[-1],
                      max(c['max_mu'] for c in m.components())) for name, m in family.items()}
    assert figures == F.FIGURES
    four, inter = family['four16'], family['four16_interleaved']
    assert four.parts == inter.parts and inter.placement == F.interleaved(64, 4)
    assert any(k == 3 for _, k, _ in family['with_k3'].parts) and any(k == 2 for _, k, _ in family['with_k3'].parts)
    assert len({m for m, _, _ in family['unequal'].parts}) > 1


def supplier(member, base, a):
    """The component whose sub-cube of the block [base, base + 2^a) holds the block's largest transient."""
    best = []
    for comp, nodes in zip(member.components(), member.placement):
        free = [j for j, node in enumerate(nodes) if node < a]
        fixed = sum(((base >> node) & 1) << j for j, node in enumerate(nodes) if node >= a)
        rows = [r for r in R._sub_cube_hist(comp, free, fixed) if r]        # cumulative counts by mu, one row per cycle state
        total = sum(r[-1] for r in rows)
        best.append(min(m for m in range(len(rows[0])) if sum(r[m] for r in rows) == total))
    top = max(best)
    return [c for c, b in enumerate(best) if b == top]


def test_different_components_supply_the_largest_transient_in_different_blocks(family):
    four = family['four16']
    blocks = [c for c in four.calls if c.count == 1 << 48 and c.max_t == INF and c.max_len == INF and not c.env]
    assert len(blocks) == 3 and any(c.first == 0 for c in blocks)
    who = {c.first: supplier(four, c.first, 48) for c in blocks}
    assert len({tuple(w) for w in who.values()}) >= 2 and all(len(w) == 1 for w in who.values()), who


def test_every_listed_call_adds_up_to_its_range(family):
    for m in family.values():
        deep = m.largest_mu_plus_lambda()
        kinds = set()
        for c in m.calls:
            assert 0 <= c.first and c.first + c.count <= 1 << m.n
            table, none, steps = m.table(c)
            assert sum(e[1] for e in table.values()) + none == c.count, (m.name, c)
            if c.max_t != INF:                                 # a cap inside the transients: many found, many not
                assert c.max_t == F.CAP[m.name] < deep and min(none, c.count - none) > c.count >> 4, (m.name, c)
                kinds.add('cap')
            if c.max_len == 1:
                assert all(e[0] == 1 for e in table.values()) and none > 0
                kinds.add('len')
            kinds.update(k for k, _ in c.env)
        assert kinds >= ({'cap', 'len'} if m.name in F.CAPPED else {'len'}), m.name
        if m.n <= 64:
            assert kinds >= {'BSX_CUBE_SPLIT', 'BSX_CUBE_DEPTH'}, m.name
    hi = family['n96']
    assert any(c.first >> 64 for c in hi.calls)
    assert any(c.first >> 64 != (c.first + c.count - 1) >> 64 for c in hi.calls)


# ---- the north star's basins, sampled ------------------------------------------------------------------------------

def test_north_star_basin_shares_of_an_oracle_sample():
    """2^16 problems drawn from random.Random(64), one oracle walk each: every attractor's share of the sample lies within
    6 sigma of its pinned exact share p = basin / 2^64, sigma = sqrt(p (1 - p) / N); every sample ends in one of the two."""
    sample, lost = F.north_star_sample()
    n = F.NORTH_STAR_SAMPLES
    assert lost == 0 and set(sample) <= set(F.NORTH_STAR) and sum(e[1] for e in sample.values()) == n
    assert sum(basin for _, basin in F.NORTH_STAR.values()) == 1 << 64
    for key, (length, basin) in F.NORTH_STAR.items():
        hits = sample.get(key, (length, 0, 0, 0))
        assert hits[0] == length
        p = basin / 2.0 ** 64
        sigma = sqrt(p * (1 - p) / n)
        print('north star {:#x}: exact share {:.6f}, sampled {:.6f}, sigma {:.6f}'.format(key, p, hits[1] / n, sigma))
        assert abs(hits[1] / n - p) <= 6 * sigma
