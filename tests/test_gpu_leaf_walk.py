"""
The depth-1 level per parent (the `P.leaf` loop of the lower build, DESIGN.md "The depth-1 level per parent") at the shapes
the rest of the suite does not reach: a cache mirror with hundreds of entries spread over many 64-slot groups of slots (a
launch of that level moves the occupied entries to the front of its mirror, 64 slots per wave and round, and walks those
alone), groups that are half full, a mirror of more slots than a workgroup has threads, work items of one or two
32-children words, and a rule table of all 64 rules.

Network family (`family_yaml`): a ring of R nodes that rotate, W layer-1 nodes that fall to 0, D layer-0 nodes whose rules
read 1-4 layer-1 / ring nodes and are 0 whenever their layer-1 inputs are 0; nobody reads layer 0.  The cycle states are
exactly "ring arbitrary, everything else 0" (2^R cached states, one attractor per binary necklace, mu <= 2), F^2 depends on
the ring digits alone, and F^1 on the ring and layer-1 digits: under a forced top depth of 2 the depth-1 level adds the W
layer-1 digits (kb = W) and has exactly the D layer-0 rules as dependent rules (the layer-1 rules are a constant 0 written
over a ring node, which is no added digit).
"""
import os
import re

import numpy as np
import pytest

from boolsi_amd.attract import merge_tables, record_ints
from boolsi_amd.compile import compile_problem
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text
from leaf_walk_family import family_yaml, necklaces

pytestmark = pytest.mark.gpu
KNOBS = ('BSX_CUBES', 'BSX_CUBE_DEPTH', 'BSX_CUBE_LEAF', 'BSX_CACHE_LDS_KB', 'BSX_DEBUG')
CAPS = ((np.inf, np.inf), (7, 2), (2, np.inf))      # (max_t, max_len); (7, .) at R = 7 and (2, .) cut between mu = 0 and mu = 1


@pytest.fixture()
def knobs():
    yield
    for k in KNOBS:
        os.environ.pop(k, None)


def engine_for(text, max_t=np.inf):
    from boolsi_amd.engine import Engine
    net, space = compile_problem(parse_input_text(text, max_t, Mode.ATTRACT))
    eng = Engine(0)
    eng.set_problem(net, space)
    return eng


def outcome(r):
    return merge_tables([r.table]), r.n_no_attractor, r.stats['state_steps']


def three_ways(eng, n, depth, max_t, max_len, capfd=None, slots=None, R=None):
    """All 2^n problems per parent, per child and by plain enumeration; the per-parent level must have run -- with
    `slots`: on a mirror of that many slots that holds all 2^R cycle states, by the library's own debug line."""
    total = 1 << n
    os.environ['BSX_CUBE_DEPTH'] = depth
    if slots:
        eng.attract2(0, total, max_t, max_len)          # (first contact with the attractors: the mirror grows with the cache)
        capfd.readouterr()
        os.environ['BSX_DEBUG'] = '1'
    a = eng.attract2(0, total, max_t, max_len)
    if slots:
        os.environ.pop('BSX_DEBUG')
        seen = re.findall(r'\[bsx\] mirror: (\d+) cycle states cached, (\d+) slots', capfd.readouterr().err)
        print('mirror lines of the per-parent run:', seen)
        assert seen and all((int(c), int(m)) == (total >> (n - R), slots) for c, m in seen)
    os.environ['BSX_CUBE_LEAF'] = '0'
    b = eng.attract2(0, total, max_t, max_len)
    os.environ.pop('BSX_CUBE_LEAF')
    os.environ['BSX_CUBES'] = '0'
    c = eng.attract2(0, total, max_t, max_len)
    os.environ.pop('BSX_CUBES')
    os.environ.pop('BSX_CUBE_DEPTH')
    print('n {} depth {} caps {} {}: lower updates per parent {} / per child {}'.format(
        n, depth, max_t, max_len, a.stats['lower_executed_steps'], b.stats['lower_executed_steps']))
    assert outcome(a) == outcome(b) == outcome(c)
    assert sum(e[1] for e in outcome(a)[0].values()) + a.n_no_attractor == total
    # one update per parent against one per child: anything else did not reach the per-parent level
    assert a.stats['lower_executed_steps'] < b.stats['lower_executed_steps']


@pytest.mark.parametrize('depth', ['2', '3'])
@pytest.mark.parametrize('R,lds_kb,slots', [(7, None, 1024), (6, None, 512), (6, 4, 256)])
def test_a_dense_mirror_over_many_chunks(knobs, capfd, R, lds_kb, slots, depth):
    """2^R cycle states plus their representative entries all over the mirror.  R = 7: 1024 slots, two rounds of the
    768-thread compaction; R = 6: 512 slots; R = 6 once more with the smallest mirror budget that still holds the 64 states,
    4 KiB = 256 slots of 16 bytes (a cube pass needs four slots per cycle state; 3 KiB gives 128): fewer slots than a round
    has threads, up to half of them occupied.  The budget is read with every set_problem, so it stays in the environment
    for the whole test; the uncapped per-parent run proves its mirror by the library's `[bsx] mirror: ... slots` line: all
    2^R cycle states cached, that many slots (under a cap only the attractors within it are ever found and cached -- 2 or
    4 states here, a 64-slot mirror -- so the capped runs check the accounting, not the dense mirror)."""
    W, D = 6, 12
    if lds_kb:
        os.environ['BSX_CACHE_LDS_KB'] = str(lds_kb)
    eng = engine_for(family_yaml(R, W, D))
    try:
        for max_t, max_len in CAPS:
            net, space = compile_problem(parse_input_text(family_yaml(R, W, D), max_t, Mode.ATTRACT))
            eng.set_problem(net, space)
            three_ways(eng, R + W + D, depth, max_t, max_len, capfd, slots if max_t == np.inf else None, R)
        full = eng.attract2(0, 1 << (R + W + D))
        neck = necklaces(R)
        assert {k: v[:2] for k, v in merge_tables([full.table]).items()} == {k: [lam, lam << (W + D)] for k, lam in neck.items()}
    finally:
        eng.close()


def test_few_parents_and_several_pieces(knobs):
    """64 parents with 1024 children each: two pieces of 512 children, shared out so that an item has one or two words."""
    R, W, D = 6, 10, 10
    eng = engine_for(family_yaml(R, W, D))
    try:
        for max_t, max_len in CAPS:
            net, space = compile_problem(parse_input_text(family_yaml(R, W, D), max_t, Mode.ATTRACT))
            eng.set_problem(net, space)
            three_ways(eng, R + W + D, '2', max_t, max_len)
    finally:
        eng.close()


@pytest.mark.parametrize('D', [33, 64])
def test_a_full_rule_table(knobs, D):
    """33 and 64 dependent rules (n = 49: two state words; n = 80: the four-word build with a full table), one aligned
    block through attract2 -- the whole space at n = 49, a block of 2^63 problems at n = 80, whose fixed digits belong to
    layer 0 and change nothing.  Against the per-child level (hash probe, not the walk), and in
    closed form: every ring value's basin is the block size / 2^R, summed per necklace; the cycle states inside the block
    (first = 0 only) have mu = 0, everybody else 1 or 2."""
    R, W = 6, 10
    n = R + W + D
    b = min(n, 63)
    first = 0 if n <= 63 else 0x15A5 << 63
    eng = engine_for(family_yaml(R, W, D))
    try:
        os.environ['BSX_CUBE_DEPTH'] = '2'
        eng.attract2(first, 1 << 30)
        a = eng.attract2(first, 1 << b)
        os.environ['BSX_CUBE_LEAF'] = '0'
        c = eng.attract2(first, 1 << b)
        print('n {}: lower updates per parent {} / per child {}'.format(n, a.stats['lower_executed_steps'], c.stats['lower_executed_steps']))
        assert outcome(a) == outcome(c)
        assert a.stats['lower_executed_steps'] < c.stats['lower_executed_steps']
        table = sorted(record_ints(r) for r in a.table)
        assert sum(r[2] for r in table) + a.n_no_attractor == 1 << b and a.n_no_attractor == 0
        assert [r[:3] for r in table] == [(k, lam, lam << (b - R)) for k, lam in sorted(necklaces(R).items())]
        for key, lam, count, s1, s2 in table:
            on_cycle = lam if first == 0 else 0
            assert count - on_cycle <= s1 <= 2 * (count - on_cycle) and s2 >= s1
    finally:
        eng.close()
