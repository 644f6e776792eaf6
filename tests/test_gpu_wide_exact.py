"""
The wide-state kernels (k_wide, networks of 257 to 1024 nodes) and the device-side reduction behind them, against
the exact reference of tests/wide_ref.py (proven against the CPU oracle at n <= 256 by tests/test_wide_ref.py).
Every comparison is exact equality on integers.

Each case has an `expect_*` function that builds its expected results from the reference alone and asserts, from
the reference alone, that the case is not vacuous (found and not found at the splitting cap, at least two attractors,
a cycle longer than 1, a transient, a target hit and a miss, two T_p).  The seeds below were chosen on the CPU so
that these hold; the tests then compare the engine with the expected results.

Columns per workgroup.  wide_set_problem_space takes the largest power of two L <= 64 with
wide_lds_words(rows, L, n_fslots, n_pv) = 4 * rows * L + (136 + 2 * (n_fslots + n_pv)) * L + 520 words within
159 KiB = 40704 words, rows = n rounded up to 64.  L is not exposed, so it is derived here and not asserted; a
group is G = 32 * L problems.
     n   rows   words at L = 16   at L = 8    L
   257    320       23176                     16   one node in state word 4, 63 padding rows   (L = 32: 45832)
   300    320       23496                     16   (six slots, four perturbation variations)
   321    384       27272                     16   ragged word
   576    576       39560                     16   last size before L drops
   577    640       43656          22088       8   first L = 8 size
   600    640       43688          22104       8   (one fixed-variation slot)
   700    704       47912          24216       8   (three slots, two perturbation variations)
  1000   1024                      34376       8
  1023   1024                      34376       8   ragged top word
  1024   1024                      34376       8   the maximum
"""
import functools
import random

import numpy as np
import pytest

from boolsi_amd import synth
from boolsi_amd.attract import merge_tables
from boolsi_amd.compile import code_to_words, compile_problem
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text
from wide_ref import WideRef, aggregate, code_of, words_of

pytestmark = pytest.mark.gpu
SIM_T = 40


# ---- networks and problem spaces (pure functions of their arguments: seeds are chosen without a GPU) ---------------

def yaml_of(preds, masks, init, fixed=None, perturbations=None):
    """BoolSi YAML of a network given as predecessor lists and truth-table masks."""
    n = len(preds)
    out = ['nodes:'] + ['    - {}'.format(synth.node_name(i)) for i in range(n)] + ['', 'update rules:']
    out += ['    {}: {}'.format(synth.node_name(i), synth.rule_text(preds[i], masks[i])) for i in range(n)]
    out += ['', 'initial state:'] + ['    {}: {}'.format(synth.node_name(i), init[i]) for i in range(n)]
    if fixed:
        out += ['', 'fixed nodes:'] + ["    {}: '{}'".format(synth.node_name(i), s) for i, s in fixed.items()]
    if perturbations:
        out += ['', 'perturbations:']
        for i, by_state in perturbations.items():
            out.append('    {}:'.format(synth.node_name(i)))
            out += ["        '{}': '{}'".format(s, times) for s, times in by_state.items()]
    return '\n'.join(out) + '\n'


def network(n, k, seed):
    """synth.random_network; for k >= 3 every table is ANDed with a second draw (a quarter of the rows true), which
    brings the dynamics from the chaotic regime of unbiased k = 3 tables to where attractors are reached within a
    few hundred steps.  A rule keeps all its k predecessors in the text, so the kernel's K follows k."""
    preds, masks = synth.random_network(n, k, seed)
    if k >= 3:
        rng = random.Random(seed + 1)
        masks = [m & rng.getrandbits(1 << k) for m in masks]
    return preds, masks


def initial(n, seed, n_any, n_high, high_from=256):
    """Seeded constant bits; n_any 'any' nodes: the last node, n_high - 1 more at index >= high_from (as many as
    there are), the rest below 256."""
    rng = random.Random(seed + 2)
    bits = synth.seeded_bits(n, seed + 3)
    high = rng.sample(range(high_from, n - 1), min(n_high - 1, n - 1 - high_from)) + [n - 1]
    any_nodes = set(high) | set(rng.sample(range(256), n_any - len(high)))
    return ['any' if i in any_nodes else str(bits[i]) for i in range(n)]


def plain_case(n, k, seed):
    """9 'any' nodes (512 problems), three of them at index >= 256 where the network has that many."""
    preds, masks = network(n, k, seed)
    return yaml_of(preds, masks, initial(n, seed, 9, 3))


def many_preds_case(seed):
    """n = 600, k = 2, except node 123 with 12 and node 300 with 9 predecessors, all but two of them above 255; node
    300 also carries the fixed-node variation '1?'.  9 'any' nodes -> 1024 problems."""
    n = 600
    preds, masks = network(n, 2, seed)
    rng = random.Random(seed + 4)
    for node, k, low in ((123, 12, 2), (300, 9, 2)):
        preds[node] = sorted(rng.sample(range(256), low) + rng.sample(range(256, n), k - low))
        masks[node] = rng.getrandbits(1 << k)
    return yaml_of(preds, masks, initial(n, seed, 9, 3), fixed={300: '1?'})


def variations_case(n, seed):
    """The variations of variations_n40 (test_gpu_wide_family.py) moved to high nodes; 6 'any' nodes.
    64 * (3 * 2 * 2) * (3 * 2) = 4608 problems; T_p = 9 where the 'any?' perturbation is present, else 7."""
    preds, masks = network(n, 2, seed)
    return yaml_of(preds, masks, initial(n, seed, 6, 3), fixed={300: 'any?', 650: '0?', 2: 'any'},
                   perturbations={640: {'1': '2, 6-7', 'any?': '9'}, 40: {'0?': '3'}})


def many_any_case(seed):
    """n = 1024 with 70 'any' nodes, 20 of them above index 900."""
    preds, masks = network(1024, 2, seed)
    return yaml_of(preds, masks, initial(1024, seed, 70, 20, 901))


def second_group_case(n, n_any, seed):
    """n_any 'any' nodes, three of them at index >= 256, and variations on the nodes from n - 40 on: six fixed-node
    variations, the lowest of them (the least significant variant digit) 'any?', and four perturbation variations
    at t = 1 .. 4.  2^n_any * 3 * 2^9 problems; T_p = 0 .. 4."""
    preds, masks = network(n, 2, seed)
    v = n - 40
    return yaml_of(preds, masks, initial(n, seed, n_any, 3),
                   fixed={v: 'any?', v + 4: '0?', v + 8: '1?', v + 12: 'any', v + 16: '0?', v + 20: '1?'},
                   perturbations={v + 24: {'0?': '1', '1?': '3'}, v + 28: {'1?': '2'}, v + 32: {'0?': '4'}})


RING_A, RING_B = [3, 17, 40, 61], [700, 767, 768, 960, 999]


def rings_case():
    """n = 1000: x_i <- the next node of its ring on rings A and B, every other node constant 0; the nine ring nodes
    are 'any'.  Node 500 starts at 1 and falls to 0 in the first step, so every problem has mu = 1."""
    n = 1000
    preds, masks, init = [[] for _ in range(n)], [0] * n, ['0'] * n
    for ring in (RING_A, RING_B):
        for j, node in enumerate(ring):
            preds[node], masks[node], init[node] = [ring[(j + 1) % len(ring)]], 0b10, 'any'
    init[500] = '1'
    return yaml_of(preds, masks, init)


# ---- shared machinery ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def compiled(text):
    """-> (net, space, reference), parsed and lowered once per input."""
    net, space = compile_problem(parse_input_text(text, 100000, Mode.SIMULATE))
    return net, space, WideRef(net, space)


@pytest.fixture(scope='module')
def eng():
    from boolsi_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def load(eng, text):
    net, space, _ = compiled(text)
    eng.set_problem(net, space)
    assert eng.wide
    return net


def expected_attract(recs):
    """Per-problem reference records -> (table, number without an attractor, reference steps)."""
    table, none = aggregate(recs)
    return table, none, sum(r[4] for r in recs)


def assert_not_vacuous(split, generous):
    """split / generous: reference records of a case at its splitting and at its generous cap."""
    n_found = sum(1 for r in split if r[0])
    assert 0 < n_found < len(split), 'the splitting cap does not split'
    found = [r for r in generous if r[0]]
    assert len({r[1] for r in found}) >= 2, 'fewer than two attractors'
    assert any(r[2] > 1 for r in found), 'no cycle longer than 1'
    assert any(r[3] > 0 for r in found), 'no transient'


def check_attract(eng, first, count, max_t, recs):
    r = eng.attract_wide(first, count, max_t)
    table, none, steps = expected_attract(recs)
    assert merge_tables([r.table]) == table
    assert r.n_no_attractor == none
    assert r.stats['state_steps'] == steps


def words_array(codes, n_words):
    """(Nested) list of state codes -> uint64 array with a last axis of n_words."""
    if isinstance(codes, int):
        return words_of(codes, n_words)
    return np.array([words_array(c, n_words) for c in codes], np.uint64)


def check_simulate(eng, net, first, count, sim, trajectories=True):
    traj, final, digest, st = eng.simulate(first, count, SIM_T, trajectories=trajectories)
    W = net.n_words
    if trajectories:
        assert np.array_equal(traj, words_array(sim[0], W))
    assert np.array_equal(final, words_array(sim[1], W))
    assert np.array_equal(digest, np.array(sim[2], np.uint64))
    assert st['state_steps'] == count * SIM_T


def target_nodes(n):
    """Five nodes, at least two of them at index >= 512 where the network has them (else >= 256): the last node (an
    'any' node in every case), n - 40, the middle of [256, n), and two low ones."""
    nodes = {5, 100, n - 1, n - 40, 256 + (n - 256) // 2}
    return sorted(nodes | {150} if len(nodes) < 5 else nodes)


def expect_target(ref, idx, traj, tp_max, max_t, nodes=None):
    """Target substate on `nodes` (default: target_nodes), its values taken from the first state
    of the reference's trajectories
    (problem by problem, from t = tp_max on) that some of the trajectories pass through and some do not.
    -> (nodes, code, [(offset, t) of the hits])"""
    nodes = nodes or target_nodes(ref.n)
    mask = sum(1 << i for i in nodes)
    sub = np.array([[c & mask for c in tr[tp_max:]] for tr in traj], object)
    for cand in dict.fromkeys(sub.ravel().tolist()):
        if 0.1 < (sub == cand).any(axis=1).mean() < 0.9:
            break
    else:
        raise AssertionError('no substate that splits the trajectories')
    res = ref.target(idx, max_t, nodes, cand)
    hits = [(q, t) for q, (reached, t) in enumerate(res) if reached]
    assert 0 < len(hits) < len(res), 'the target has no hit or no miss'
    return nodes, cand, hits


def check_target(eng, net, first, count, max_t, target):
    nodes, code, ref_hits = target
    mask = code_to_words(sum(1 << i for i in nodes), net.n_words)
    codew = code_to_words(code, net.n_words)
    hits, _ = eng.target(first, count, max_t, mask, codew)
    assert [(int(h['offset']), int(h['t'])) for h in hits] == ref_hits
    n_hits, hist, listed, _ = eng.target_summary(first, count, max_t, mask, codew, hist_bins=8, cap=5)
    assert n_hits == len(ref_hits)
    assert [(int(h['offset']), int(h['t'])) for h in listed] == ref_hits[:5]
    assert hist.tolist() == [sum(1 for _, t in ref_hits if t == b) for b in range(7)] + \
        [sum(1 for _, t in ref_hits if t >= 7)]


# ---- per size, k = 2 and k = 3: problems 5 .. 504 of 512 (a ragged group at L = 16; two groups, the second ragged,
#      at L = 8) -----------------------------------------------------------------------------------------------------

FIRST, COUNT, GENEROUS = 5, 500, 300
PLAIN = {       # (n, k): (seed, splitting cap), chosen with the reference: see assert_not_vacuous
    (257, 2): (8, 30), (257, 3): (6, 114), (321, 2): (2, 52), (321, 3): (10, 30),
    (576, 2): (10, 203), (576, 3): (2, 42), (577, 2): (31, 33), (577, 3): (1, 54),
    (1023, 2): (11, 41), (1023, 3): (7, 57), (1024, 2): (3, 34), (1024, 3): (4, 55),
}
PLAIN_IDS = ['n{}_k{}'.format(n, k) for n, k in PLAIN]


def plain_text(n, k):
    return plain_case(n, k, PLAIN[n, k][0])


@functools.lru_cache(maxsize=None)
def expect_plain_attract(n, k):
    ref = compiled(plain_text(n, k))[2]
    idx = range(FIRST, FIRST + COUNT)
    split, generous = ref.attract(idx, PLAIN[n, k][1])[0], ref.attract(idx, GENEROUS)[0]
    assert_not_vacuous(split, generous)
    return split, generous


@functools.lru_cache(maxsize=None)
def expect_plain_simulate(n, k):
    ref = compiled(plain_text(n, k))[2]
    idx = range(FIRST, FIRST + COUNT)
    sim = ref.simulate(idx, SIM_T)
    return sim, expect_target(ref, idx, sim[0], 0, SIM_T)


@pytest.mark.parametrize('n,k', list(PLAIN), ids=PLAIN_IDS)
def test_attract_at_a_splitting_and_a_generous_cap(eng, n, k):
    split, generous = expect_plain_attract(n, k)
    load(eng, plain_text(n, k))
    assert eng.network_info()['mux_slots'] == k
    check_attract(eng, FIRST, COUNT, PLAIN[n, k][1], split)
    check_attract(eng, FIRST, COUNT, GENEROUS, generous)


@pytest.mark.parametrize('n,k', list(PLAIN), ids=PLAIN_IDS)
def test_simulate_and_target(eng, n, k):
    sim, target = expect_plain_simulate(n, k)
    net = load(eng, plain_text(n, k))
    check_simulate(eng, net, FIRST, COUNT, sim)
    check_target(eng, net, FIRST, COUNT, SIM_T, target)


# ---- n = 600: nodes with 9 and 12 predecessors (KW = true), predecessor indices above 255, one of them with a
#      fixed-node variation; problems 5 .. 704 of 1024 run into the variant digit ------------------------------------

PREDS_SEED, PREDS_SPLIT, PREDS_FIRST, PREDS_COUNT = 6, 95, 5, 700


@functools.lru_cache(maxsize=None)
def expect_many_preds():
    net, space, ref = compiled(many_preds_case(PREDS_SEED))
    assert sorted(len(p) for p in net.predecessor_lists)[-2:] == [9, 12]
    assert sum(1 for i in (123, 300) for p in net.predecessor_lists[i] if p > 255) == 17
    assert space.n_problems == 1024 and space.fixed_var.tolist() == [[300, 1]]
    idx = range(PREDS_FIRST, PREDS_FIRST + PREDS_COUNT)
    split, generous = ref.attract(idx, PREDS_SPLIT)[0], ref.attract(idx, GENEROUS)[0]
    assert_not_vacuous(split, generous)
    sim = ref.simulate(idx, SIM_T)
    return split, generous, sim, expect_target(ref, idx, sim[0], 0, SIM_T)


def test_nodes_with_9_and_12_predecessors_at_600_nodes(eng):
    split, generous, sim, target = expect_many_preds()
    net = load(eng, many_preds_case(PREDS_SEED))
    check_attract(eng, PREDS_FIRST, PREDS_COUNT, PREDS_SPLIT, split)
    check_attract(eng, PREDS_FIRST, PREDS_COUNT, GENEROUS, generous)
    check_simulate(eng, net, PREDS_FIRST, PREDS_COUNT, sim)
    check_target(eng, net, PREDS_FIRST, PREDS_COUNT, SIM_T, target)


# ---- n = 700 and n = 1024: fixed-node and perturbation variations on nodes above 255 --------------------------------

VARIATIONS = {700: (5, 30, 100), 1024: (3, 34, 100)}      # n: (seed, splitting cap, generous cap)
VAR_SPACE = 4608
# the whole space; a range whose flat index carries from the six 'any' digits into the variant number several times,
# and across problem 1536, from where on the 'any?' perturbation at t = 9 is present (it is the most significant
# digit, and 1536 is a multiple of the group size, so only this range has a group with two T_p); the last 777 problems
VAR_RANGES = [(0, VAR_SPACE), (1536 - 100, 300), (VAR_SPACE - 777, 777)]


@functools.lru_cache(maxsize=None)
def expect_variations(n):
    seed, split_cap, generous_cap = VARIATIONS[n]
    net, space, ref = compiled(variations_case(n, seed))
    assert space.n_problems == VAR_SPACE and len(space.any_nodes) == 6
    idx = range(VAR_SPACE)
    tps = [ref.problem(i).tp for i in idx]
    first, count = VAR_RANGES[1]            # its first group (256 problems at L = 8) has two T_p
    assert set(tps[first:first + 100]) == {7} and set(tps[first + 100:first + 256]) == {9}
    # one reference run over the whole space; the other ranges are slices of its per-problem records
    split, generous = ref.attract(idx, split_cap)[0], ref.attract(idx, generous_cap)[0]
    assert_not_vacuous(split, generous)
    for first, count in VAR_RANGES:
        assert_not_vacuous(split[first:first + count], generous[first:first + count])
    # some problem closes its cycle within split_cap steps of its T_p but not by t = split_cap: the cap counts from 0
    assert any(split_cap < g[4] <= split_cap + tp for g, tp in zip(generous, tps) if g[0])
    first, count = VAR_RANGES[2]
    tail = range(first, first + count)
    sim = ref.simulate(tail, SIM_T)
    # target on the nodes that carry the variations: trajectories with other fixed values never pass through it
    return split, generous, sim, expect_target(ref, tail, sim[0], max(tps), SIM_T, [2, 40, 300, 640, 650])


@pytest.mark.parametrize('n', list(VARIATIONS))
def test_variations_at_high_nodes(eng, n):
    split, generous, sim, target = expect_variations(n)
    seed, split_cap, generous_cap = VARIATIONS[n]
    net = load(eng, variations_case(n, seed))
    for first, count in VAR_RANGES:
        check_attract(eng, first, count, split_cap, split[first:first + count])
        check_attract(eng, first, count, generous_cap, generous[first:first + count])
    first, count = VAR_RANGES[2]
    check_simulate(eng, net, first, count, sim)
    check_target(eng, net, first, count, SIM_T, target)


# ---- n = 1024, 70 'any' nodes: the flat index carries from first_digits[0] into [1] ---------------------------------

ANY_SEED, ANY_SPLIT, ANY_COUNT = 8, 72, 300
ANY_FIRSTS = [(1 << 64) - 100, (1 << 69) + 12345]


@functools.lru_cache(maxsize=None)
def expect_many_any():
    net, space, ref = compiled(many_any_case(ANY_SEED))
    assert len(space.any_nodes) == 70 and sum(1 for a in space.any_nodes.tolist() if a > 900) == 20
    out = []
    for first in ANY_FIRSTS:
        idx = range(first, first + ANY_COUNT)
        split, generous = ref.attract(idx, ANY_SPLIT)[0], ref.attract(idx, GENEROUS)[0]
        assert_not_vacuous(split, generous)
        out.append((split, generous, ref.simulate(idx, SIM_T)))
    return out


def test_more_than_64_any_nodes(eng):
    expected = expect_many_any()
    net = load(eng, many_any_case(ANY_SEED))
    for first, (split, generous, sim) in zip(ANY_FIRSTS, expected):
        check_attract(eng, first, ANY_COUNT, ANY_SPLIT, split)
        check_attract(eng, first, ANY_COUNT, GENEROUS, generous)
        check_simulate(eng, net, first, ANY_COUNT, sim)


# ---- n = 1023: trajectories with scattered offsets and per-problem lengths ------------------------------------------

@functools.lru_cache(maxsize=None)
def expect_scattered():
    ref = compiled(plain_text(1023, 2))[2]
    rng = random.Random(1023)
    offsets = rng.sample(range(500), 40)
    t_len = [0, 60] + [rng.randrange(61) for _ in range(38)]
    rng.shuffle(t_len)
    assert offsets != sorted(offsets) and {0, 60} <= set(t_len)
    return offsets, t_len, ref.trajectories([7 + o for o in offsets], t_len)


def test_trajectories_with_scattered_offsets_and_lengths(eng):
    offsets, t_len, expected = expect_scattered()
    net = load(eng, plain_text(1023, 2))
    trajs, st = eng.trajectories(7, offsets, t_len)
    assert len(trajs) == 40
    for got, want in zip(trajs, expected):
        assert np.array_equal(got, words_array(want, net.n_words))
    assert st['state_steps'] == sum(t_len)


# ---- key order at n = 1000: two rings, one in state word 0, one in words 10 to 15 -----------------------------------

def necklaces(ring):
    out = {}
    for v in range(1 << ring):
        orbit = {((v >> r) | (v << (ring - r))) & ((1 << ring) - 1) for r in range(ring)}
        out.setdefault(min(orbit), len(orbit))
    return out          # key -> cycle length


def spread(value, ring):
    """Ring value (bit j = the ring's j-th node) -> state code."""
    return sum(((value >> j) & 1) << node for j, node in enumerate(ring))


def rot(value, r, ring):
    r %= ring
    return ((value >> r) | (value << (ring - r))) & ((1 << ring) - 1)


RING_CAPS = (100, 10)        # generous; splitting: found iff 1 + lambda <= 10 (lambda is 1, 2, 4, 5, 10 or 20)


def rings_closed_form(cap):
    """A state is (a, b), the values of the two rings; a step rotates both by one place.  The cycle of (a, b) has
    lcm(|a|, |b|) states, |x| the size of x's orbit.  Ring B holds the higher nodes, so the minimum of a cycle has
    the smallest b of b's orbit, and among the cycle's states with that b, which are |b| steps apart, the smallest
    a.  Every problem is one (a, b) with node 500 set, which is on no cycle and one step away from (a, b) rotated:
    mu = 1, T_p = 0, count = cycle length, found iff 1 + lambda <= cap.
    -> (table, number without an attractor, reference steps)"""
    nb, table, none, steps = necklaces(len(RING_B)), {}, 0, 0
    for b, lb in nb.items():
        for a in range(1 << len(RING_A)):
            orbit = [rot(a, lb * s, len(RING_A)) for s in range(len(RING_A))]
            lam = int(np.lcm(len({rot(a, s, len(RING_A)) for s in range(len(RING_A))}), lb))
            if 1 + lam <= cap:
                table[spread(b, RING_B) | spread(min(orbit), RING_A)] = [lam, lam, lam, lam]
                steps += lb * (1 + lam)
            else:
                none += lb
                steps += lb * cap
    return table, none, steps


@functools.lru_cache(maxsize=None)
def expect_rings():
    ref = compiled(rings_case())[2]
    out = {}
    for cap in RING_CAPS:
        recs, steps = ref.attract(range(512), cap)
        out[cap] = expected_attract(recs)
        assert out[cap] == rings_closed_form(cap) and out[cap][2] == steps
    assert_not_vacuous(ref.attract(range(512), RING_CAPS[1])[0], ref.attract(range(512), RING_CAPS[0])[0])
    # non-vacuity: the node that decides between the minimum and another state of its cycle (the highest node in
    # which they differ) lies below 64 for some cycle (ring B uniform) and at or above 960 for another
    deciding = set()
    for key, e in out[RING_CAPS[0]][0].items():
        s = np.array([[(key >> i) & 1 for i in range(ref.n)]], np.uint8)
        for _ in range(e[0] - 1):
            s = ref.rules(s)
            deciding.add((key ^ code_of(s[0])).bit_length() - 1)
    assert min(deciding) < 64 and max(deciding) >= 960
    return out


def test_key_order_with_rings_in_low_and_high_words(eng):
    expected = expect_rings()
    load(eng, rings_case())
    for cap, (table, none, steps) in expected.items():
        r = eng.attract_wide(0, 512, cap)
        assert merge_tables([r.table]) == table
        assert r.n_no_attractor == none and r.stats['state_steps'] == steps


# ---- a workgroup's second group -------------------------------------------------------------------------------------
# The grid of a k_wide launch is min(groups, CUs * per_cu) blocks and per_cu = 1 for every wide network, so a block
# runs a second group only above CUs * 32 * L problems.  The space has as many 'any' nodes as a group has problems
# (2^8 at L = 8, 2^9 at L = 16), so that every group of a range that starts at a multiple of G is one variant, and
# the least significant variant digit, the 'any?' fixed node, is (first / G + group) mod 3.  `first` is chosen so
# that, where CUs is no multiple of 3, block 0 runs a group with that node fixed to 1 and then one without it: masks
# left over from a block's first group would show in its second.  3 * 2^9 variants: enough problems up to 512 CUs.

SECOND = {1024: (8, 8, 3, 36), 300: (16, 9, 2, 33)}             # n: (L, 'any' nodes, seed, cap that splits the sample)
SECOND_SIM_T = 24


def second_group_sample(cus, L):
    """-> (first, count, sampled offsets): every problem of the first group that is a block's second, every problem
    of the last, ragged group, and seeded others from the rest, 512 in all (more where those two groups alone are
    more)."""
    G = 32 * L
    count = cus * G + G + 77
    must = list(range(cus * G, count))
    rng = random.Random(cus)
    return (-cus % 3) * G, count, sorted(must + rng.sample(range(cus * G), max(512 - len(must), 64)))


@functools.lru_cache(maxsize=None)
def expect_second_group(n, cus):
    L, n_any, seed, cap = SECOND[n]
    net, space, ref = compiled(second_group_case(n, n_any, seed))
    assert 32 * L == 1 << n_any and space.fixed_var[0].tolist() == [n - 40, 3]
    first, count, sample = second_group_sample(cus, L)
    assert first + count <= space.n_problems
    idx = [first + o for o in sample]
    if cus % 3:                 # block 0: node n - 40 fixed to 1 in its first group, not fixed in its second
        assert ref.problem(first).fmask[n - 40] and ref.problem(first).fval[n - 40]
        second = first + cus * 32 * L
        assert not ref.problem(second).fmask[n - 40]
        # ... and it matters there: the same problem with the node fixed to 1 (digit 2 instead of 0) ends elsewhere
        assert ref.simulate([second], SECOND_SIM_T)[2] != ref.simulate([second + 2 * 32 * L], SECOND_SIM_T)[2]
    assert len({ref.problem(i).tp for i in idx}) >= 2
    traj, final, digest = ref.simulate(idx, SECOND_SIM_T)
    recs = ref.attract(idx, cap)[0]
    assert_not_vacuous(recs, recs)
    return first, count, sample, final, digest, aggregate(recs)[0]


@pytest.mark.parametrize('n', list(SECOND))
def test_a_workgroups_second_group(eng, n):
    cus = eng.device_info()['compute_units']        # hipDeviceProp_t::multiProcessorCount, which sizes the grid
    if cus > 512:
        pytest.skip('{} compute units: the problem space of this case ends at 512'.format(cus))
    L, n_any, seed, cap = SECOND[n]
    first, count, sample, ref_final, ref_digest, ref_table = expect_second_group(n, cus)
    net = load(eng, second_group_case(n, n_any, seed))
    _, final, digest, _ = eng.simulate(first, count, SECOND_SIM_T, trajectories=False)
    assert np.array_equal(final[sample], words_array(ref_final, net.n_words))
    assert np.array_equal(digest[sample], np.array(ref_digest, np.uint64))
    # one call in which blocks run a second group == calls in which none does
    whole = eng.attract_wide(first, count, cap)
    step = cus * 32 * L
    parts = [eng.attract_wide(first + at, min(step, count - at), cap) for at in range(0, count, step)]
    table = merge_tables([whole.table])
    assert table == merge_tables([p.table for p in parts])
    assert whole.n_no_attractor == sum(p.n_no_attractor for p in parts)
    assert whole.stats['state_steps'] == sum(p.stats['state_steps'] for p in parts)
    for key, (length, n_sampled, _, _) in ref_table.items():
        assert key in table and table[key][0] == length and table[key][1] >= n_sampled
