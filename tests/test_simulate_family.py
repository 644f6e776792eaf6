"""
CPU proof of what the members of tests/simulate_family.py claim, which tests/test_gpu_simulate_exact.py runs on the GPU, by
the oracle alone: every range has the shape and the route it claims, the states still move at the last step, every
scheduled override changes a row, the upper truth-table word of the K = 6 member matters, the mixed network has the
in-degrees and the unsorted lists it is for, variants differ in their last perturbation time, and the trajectory lists hold
the repeats, descents and short lengths they are for.

These are conditions on the reference, not measurements of the engine: a member that misses one gets other inputs.
"""
import re

import numpy as np
import pytest

from boolsi_amd.compile import compile_network
from simulate_family import (BY_NAME, EDGES, FAMILY, PER_LANE, SECOND_PASS, SLICED, SLICED64, TRAJ_MEMBERS, TRAJ_TP, VAR_TP, CORES,
                             t_lens, without_schedule_entries)

RANGES = [(mb, r) for mb in FAMILY for r in mb.ranges]
RANGE_IDS = ['{}-{}'.format(mb.name, i) for mb in FAMILY for i in range(len(mb.ranges))]


def route_by_shape(net, space, count, max_t):
    """bsx_run_simulate's rule for a call that asks for final states alone, without knobs"""
    k_mux = max(1, max(len(p) for p in net.predecessor_lists))
    rows = (net.n_nodes + 15) & ~15
    if len(space.fixed_var) or len(space.pert_var) or k_mux > 6 or count < 2048 or max_t < 64 or rows * 136 * 4 > 160 * 1024:
        return PER_LANE
    return SLICED64 if k_mux <= 3 and rows <= 128 else SLICED


@pytest.mark.parametrize('member,r', RANGES, ids=RANGE_IDS)
def test_ranges_have_the_shape_and_the_route_they_claim(member, r):
    net, space = member.compiled()
    variant = 1 << len(space.any_nodes)
    end = r.first + r.count
    assert r.count >= 1 and end <= space.n_problems and r.count <= 4096 + 37
    assert set(r.claims) <= {'ragged', 'unaligned', 'crosses', 'tp_differs'} and 'ragged' in r.claims
    assert r.count % 64 and r.count % 512 and (r.route == PER_LANE or r.count % 2048)
    if member.name != 'w5':             # (a space of 32 problems: the range starts at 3)
        assert 'unaligned' in r.claims
    if 'unaligned' in r.claims:
        assert r.first % 64
    if 'crosses' in r.claims:
        assert r.first // variant < (end - 1) // variant
    if 'tp_differs' in r.claims:
        orc = member.oracle()
        tps = {max([0] + [int(t) for t, _, _ in orc.problem(i)[4]]) for i in range(r.first, end)}
        print('{}: last perturbation times {}'.format(member.name, sorted(tps)))
        assert len(tps) >= 2 and max(tps) == VAR_TP == space.last_perturbation_t
    for max_t in member.max_ts:
        assert max_t >= space.last_perturbation_t
        assert route_by_shape(net, space, r.count, max_t) == r.route, max_t
    if r.route == PER_LANE:
        assert r.count <= 700
    else:
        assert all(64 <= t <= 130 for t in member.max_ts)
    if member.name.startswith('var_'):
        assert 'crosses' in r.claims and any('tp_differs' in q.claims for q in member.ranges)


@pytest.mark.parametrize('member,r', RANGES, ids=RANGE_IDS)
def test_the_states_still_move_at_the_last_step(member, r):
    for max_t in member.max_ts:
        final, digest = member.reference(r.first, r.count, max_t)
        before, _ = member.reference(r.first, r.count, max_t - 1)
        moving = int((final != before).any(axis=1).sum())
        distinct = len(np.unique(final, axis=0))
        print('{} max_t {}: {} of {} problems change state at the last step, {} distinct final states'.format(
            member.name, max_t, moving, r.count, distinct))
        assert moving >= 1 and distinct >= 2 and len(np.unique(digest)) >= 2


def test_names_tell_the_network():
    for mb in FAMILY:
        net, _ = mb.compiled()
        n = re.search(r'(?:^|_)[nw](\d+)', mb.name)
        k = re.search(r'(?:^|_)k(\d+)', mb.name)
        if n:
            assert net.n_nodes == int(n.group(1)), mb.name
        if k:
            assert max(len(p) for p in net.predecessor_lists) == int(k.group(1)), mb.name
    assert [mb.compiled()[0].n_words for mb in FAMILY[:11]] == [1, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4]      # 64-bit words: w64 = 3 at n = 129 and 192
    assert {SLICED, SLICED64, PER_LANE} == {mb.kind for mb in FAMILY} == set(SECOND_PASS)
    fx = BY_NAME['g2_fixed_n40'].compiled()[1].fixed.tolist()
    assert sorted(v for _, v in fx) == [0, 1]


@pytest.mark.parametrize('member', EDGES, ids=str)
def test_every_scheduled_override_changes_a_row(member):
    from oracle.cpu_oracle import Oracle
    net, space = member.compiled()
    (r,), (max_t,) = member.ranges, member.max_ts
    sched = [tuple(row) for row in space.sched.tolist()]
    times = sorted({t for t, _, _ in sched})
    assert times[0] == 1 and times[-1] == max_t == space.last_perturbation_t
    assert any(t % 2 for t in times) and any(not t % 2 for t in times[:-1])
    assert {10, 11, 12, 13} <= set(times)
    assert any({(t, 0), (t, 1)} <= {(t2, v) for t2, _, v in sched} for t in times)       # two nodes at one time, both values
    if member.kind == SLICED64:
        assert net.n_nodes == 128 and {node >> 3 for _, node, _ in sched} >= {0, 15}     # rows of wave 0 and of wave 15
        assert any(node >> 3 == 15 and t == max_t for t, node, _ in sched) and any(node >> 3 == 0 and t == 1 for t, node, _ in sched)
    for entry in sched:
        t, node, _ = entry
        with_it, _ = member.reference(r.first, r.count, t)
        without = Oracle(net, without_schedule_entries(space, lambda *row: row == entry)).simulate(
            r.first, r.count, t, want_traj=False, n_threads=CORES)[1]
        bit = (with_it[:, node >> 6] ^ without[:, node >> 6]) >> np.uint64(node & 63) & np.uint64(1)
        print('{}: the override of node {} at t = {} changes {} of {} problems'.format(member.name, node, t, int(bit.sum()), r.count))
        assert bit.any()


def test_the_upper_table_word_of_the_k6_member_matters():
    from oracle.cpu_oracle import Oracle
    member = BY_NAME['g1_k6_n40']
    net, space = member.compiled()
    low = (1 << 32) - 1
    assert all(len(p) == 6 for p in net.predecessor_lists)
    assert sum((m >> 32) != (m & low) for m in net.tt_masks) >= 30
    folded = compile_network(net.predecessor_lists, [(m & low) | ((m & low) << 32) for m in net.tt_masks])
    (r,) = member.ranges
    for max_t in member.max_ts:
        final, _ = member.reference(r.first, r.count, max_t)
        other = Oracle(folded, space).simulate(r.first, r.count, max_t, want_traj=False, n_threads=CORES)[1]
        differ = int((final != other).any(axis=1).sum())
        print('max_t {}: {} of {} final states change when the upper table word is replaced by the lower'.format(max_t, differ, r.count))
        assert differ >= r.count // 2


@pytest.mark.parametrize('member', [mb for mb in FAMILY if mb.written], ids=str)
def test_mixed_networks_have_the_degrees_and_the_unsorted_lists(member):
    net, _ = member.compiled()
    written, masks = member.written
    parsed = net.predecessor_lists
    degrees = {len(p) for p in parsed}
    kmax = 3 if 'mixed03' in member.name else 6
    assert {0, 1, kmax} <= degrees and max(degrees) == (9 if 'mixed9' in member.name else kmax)
    assert parsed[1] == [1]                                     # the self-loop
    assert all(p == sorted(w) for p, w in zip(parsed, written))
    # written in another order than parsed, and the order matters: the parsed table is not the written one
    moved = [i for i, w in enumerate(written) if w != sorted(w) and net.tt_masks[i] != masks[i]]
    print('{}: in-degrees {}, {} lists written unsorted with a table that changes under the sort'.format(member.name, sorted(degrees), len(moved)))
    assert len(moved) >= 5
    assert sum(len(p) < kmax for p in parsed) >= 10             # tables to replicate over unused select inputs


@pytest.mark.parametrize('member', TRAJ_MEMBERS, ids=str)
def test_trajectory_lists_hold_what_they_are_for(member):
    from oracle.cpu_oracle import Oracle
    net, space = member.compiled()
    first, offsets, t_len = member.traj_list
    tp_max = space.last_perturbation_t
    assert tp_max == (VAR_TP if member.name.startswith('var_') else TRAJ_TP)
    assert len(offsets) == len(t_len) == 700 and first % 64 and first + max(offsets) < space.n_problems
    assert len(set(offsets)) < len(offsets)                                         # a repeated offset
    assert any(a > b for a, b in zip(offsets, offsets[1:]))                         # a descending pair
    assert set(t_len) == set(t_lens(tp_max)) and 0 in t_len
    if member.name.startswith('var_'):
        variant = 1 << len(space.any_nodes)
        assert len({(first + o) // variant for o in offsets}) >= 3
    # a length below tp_max on a problem whose later perturbations change its states
    found = 0
    for o, t in zip(offsets[:60], t_len[:60]):
        if t >= tp_max:
            continue
        late = Oracle(net, without_schedule_entries(space, lambda t2, *_: t2 > t)).trajectory(first + o, tp_max)
        full = member.trajectory(first + o, tp_max)
        assert np.array_equal(late[:t + 1], full[:t + 1])
        assert np.array_equal(member.trajectory(first + o, t), full[:t + 1])         # a shorter run is a prefix of a longer one
        found += not np.array_equal(late, full)
    print('{}: {} short trajectories whose later perturbations change a state'.format(member.name, found))
    assert found >= 3
