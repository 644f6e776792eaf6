"""
CPU proof of what the members of tests/target_family.py claim, which tests/test_gpu_target_exact.py runs on the GPU, by
the oracle alone over the union of each member's ranges: the target is neither unreachable nor trivially reached, first
hits are spread over several times the kernel has to step to, a hit lies exactly at the time cap where the member says
so, cube passes have irrelevant digits to collapse, and every range has the shape it claims.

These are conditions on the reference, not measurements of the engine: a member that misses one gets other inputs.
"""
from math import inf

import numpy as np
import pytest

from target_family import FAMILY, N_FUZZ, fuzz_member


def times(member, max_t):
    """(number of problems, first-hit times of the reached ones) over the member's ranges"""
    n = sum(r.count for r in member.ranges)
    return n, np.concatenate([member.reference(r.first, r.count, max_t)[1] for r in member.ranges])


def sensitive(tt, k, j):
    return any(((tt >> x) ^ (tt >> (x ^ (1 << j)))) & 1 for x in range(1 << k))


def relevant_nodes(net, fixed=()):
    """nodes some rule of a node that is not fixed reads and is sensitive to"""
    preds, masks = net.predecessor_lists, net.tt_masks
    return {p for i in range(net.n_nodes) if i not in fixed for j, p in enumerate(preds[i]) if sensitive(masks[i], len(preds[i]), j)}


@pytest.mark.parametrize('member,max_t', [(mb, t) for mb in FAMILY for t in mb.max_ts], ids=str)
def test_the_target_is_neither_trivial_nor_unreachable(member, max_t):
    n, t = times(member, max_t)
    share, at0, late = len(t) / n, int((t == 0).sum()) / n, int((t >= 2).sum()) / n
    distinct = np.unique(t)
    print('{} max_t {}: reached {:.1%}, at t = 0 {:.1%}, at t >= 2 {:.1%}, {} distinct first-hit times, latest {}'.format(
        member.name, max_t, share, at0, late, len(distinct), int(t.max())))
    assert 0.05 <= share <= 0.95
    if max_t == 1:          # no time t >= 2 exists under this cap: both times that do exist must occur
        assert distinct.tolist() == [0, 1]
    else:
        assert late >= 0.01
        assert len(distinct) >= 3
    if member.at_cap and max_t != inf:
        assert (t == max_t).any()
        n1, t1 = times(member, max_t + 1)
        assert (t1 == max_t + 1).any()          # unreached under max_t (it would have stopped earlier), reached one step later
        assert int((t1 <= max_t).sum()) == len(t)
    if member.cubes_expected:
        assert 0.01 <= at0 < 1.0


@pytest.mark.parametrize('member', [mb for mb in FAMILY if mb.cubes_expected], ids=str)
def test_cube_members_have_digits_to_collapse(member):
    _, cfg, net, space, _, _ = member.compiled()
    assert len(space.any_nodes) == net.n_nodes == 20 and space.any_nodes.tolist() == list(range(20))     # nothing constant in a block but its high digits
    low16 = set(range(16))
    free = low16 - relevant_nodes(net)
    print('{}: irrelevant among the low 16 digits: {}'.format(member.name, sorted(free)))
    assert len(free) >= 2
    in_free, in_rel = [i for i in member.nodes if i in free], [i for i in member.nodes if i not in free]
    if member.name == 'leaves_leaf':
        assert in_free and not [i for i in in_rel if i < 16]
    if member.name == 'leaves_core':
        assert in_rel and not in_free
    if member.name in ('leaves_both', 'leaves_knock_out', 'leaves_fixed_point'):
        assert in_free and in_rel
    if member.name == 'leaves_knock_out':
        (node, _), = space.fixed_var.tolist()
        assert any(node in net.predecessor_lists[i] for i in range(12, 20))       # a leaf reads the knocked-out node
        other = low16 - relevant_nodes(net, fixed=(node,))
        print('  under the knock-out of node {}: {}'.format(node, sorted(other)))
        assert other != free and len(other) >= 2
    if member.name == 'leaves_fixed_point':
        from oracle.cpu_oracle import Oracle
        r = member.star[0]
        assert int(Oracle(net, space).trajectory(r, 1)[1][0]) == r and not (r >> 12) & 0xF
        (first, count, _), _ = member.ranges
        off, t = member.reference(first, count, inf)
        mine = (off & np.uint64(0xFFF)) == np.uint64(r & 0xFFF)      # the class of r: the members differ in the leaf digits 12-15
        assert sorted(set(t[mine].tolist())) == [0, 1] and int(mine.sum()) == 16


@pytest.mark.parametrize('member', [mb for mb in FAMILY if mb.chain], ids=str)
def test_chain_closed_form_equals_the_oracle(member):
    for max_t in member.max_ts + (0, 7, 19, 20, 21):
        for r in member.ranges:
            off, t = member.reference(r.first, r.count, max_t)
            coff, ct = member.closed_form(r.first, r.count, max_t)
            assert np.array_equal(off, coff) and np.array_equal(t, ct)


@pytest.mark.parametrize('member', FAMILY, ids=str)
def test_ranges_have_the_shape_they_claim(member):
    _, _, net, space, _, _ = member.compiled()
    variant = 1 << len(space.any_nodes)
    total = sum(r.count for r in member.ranges)
    assert all(r.count <= 1 << 18 and r.first + r.count <= space.n_problems for r in member.ranges)
    for r in member.ranges:
        end = r.first + r.count
        assert set(r.claims) <= {'crosses', 'unaligned', 'edge', 'block'}
        if 'crosses' in r.claims:
            assert r.first // variant < (end - 1) // variant         # a multiple of the variant size strictly inside
        if 'unaligned' in r.claims:
            assert r.first % 64 and end % 64
        if 'edge' in r.claims:
            assert r.count > 4096 and r.count % 4096 in (1, 4095)
        if 'block' in r.claims:
            assert r.first % (1 << 16) == 0 and r.count == 1 << 17
    if member.cubes_expected:
        assert any('block' in r.claims for r in member.ranges) or member.name == 'leaves_fixed_point'
    if 'variants' in member.name or 'perturbed' in member.name or 'knock_out' in member.name:
        assert any('crosses' in r.claims and 'unaligned' in r.claims for r in member.ranges)
    assert total <= 1 << 19


def test_words_and_rule_classes():
    """the kernel instantiations the members are for: state words from the node count, mux class from the widest rule"""
    shape = {mb.name: (mb.compiled()[2].n_nodes, max(len(p) for p in mb.compiled()[2].predecessor_lists)) for mb in FAMILY}
    assert shape['n20_k2'] == (20, 2) and shape['n40_k3_variants'] == (40, 3) and shape['n100_k2'] == (100, 2)
    assert shape['n200_k4'] == (200, 4) and shape['n24_k9'] == (24, 9) and shape['n48_k6'] == (48, 6) and shape['n33_perturbed'][0] == 33
    by = {mb.name: mb for mb in FAMILY}
    assert {i >> 5 for i in by['n100_k2'].nodes} == {1, 2, 3} and {0, 4, 6} <= {i >> 5 for i in by['n200_k4'].nodes}
    assert {i >> 5 for i in by['n40_k3_variants'].nodes} == {0, 1} and 32 in by['n33_perturbed'].nodes
    assert sorted(by['n40_k3_variants'].compiled()[3].radices[18:]) == [2, 2, 3] and len(by['n40_k3_variants'].compiled()[3].any_nodes) == 18
    sp = by['n33_perturbed'].compiled()[3]
    assert len(sp.sched) >= 3 and len(sp.pert_var) == 2 and sp.n_problems == 6 << 14


def test_most_fuzz_cases_have_a_late_hit():
    late = []
    for seed in range(N_FUZZ):
        mb = fuzz_member(seed)
        (first, count, _), = mb.ranges
        assert count <= 1 << 17 and 16 <= mb.compiled()[2].n_nodes <= 70
        off, t = mb.reference(first, count, mb.max_ts[0])
        late.append(bool((t >= 2).any()))
        print('fuzz {}: n {}, {} problems, max_t {}, reached {:.1%}, latest first hit {}'.format(
            seed, mb.compiled()[2].n_nodes, count, mb.max_ts[0], len(t) / count, int(t.max()) if len(t) else '-'))
    assert sum(late) >= 20
