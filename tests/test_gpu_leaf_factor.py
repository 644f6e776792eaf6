"""
The per-parent level's factorised count (boolsi_amd/csrc/bsx_leaf.h; DESIGN.md "The depth-1 level per parent") on the GPU:
every member of tests/leaf_factor_family.py -- no entangled digit, a few, the bench's six of twelve, all of them, several
pieces and parts, fewer children than a word, rules of three and four inputs -- through the three-way comparison of
tests/test_gpu_leaf_walk.py: per parent, per child (BSX_CUBE_LEAF=0) and plain enumeration (BSX_CUBES=0), under its three
caps, with a forced top depth of 2 and the first index 0, so that the cycle states inside the block exercise the mu = 0
correction.  The library's debug line must show the member's kb and m.  tests/test_leaf_factor_family.py proves on the
CPU that the members are what they claim.
"""
import os
import re

import pytest

from boolsi_amd.attract import record_ints
from boolsi_amd.compile import compile_problem
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text
from leaf_factor_family import FAMILY, R, WIDE, necklaces
from test_gpu_leaf_walk import CAPS, engine_for, knobs, outcome, three_ways  # noqa: F401  (knobs: the fixture)

pytestmark = pytest.mark.gpu
LINE = re.compile(r'\[bsx\] per-parent level: kb (\d+), (\d+) enumerated rules, (\d+) free rules, m (\d+)')


def debug_lines(capfd, member):
    seen = [tuple(int(v) for v in g) for g in LINE.findall(capfd.readouterr().err)]
    print('per-parent lines:', sorted(set(seen)), 'x', len(seen))
    assert seen and all((kb, m) == (member.W, member.m) and n_enum + n_free == member.D for kb, n_enum, n_free, m in seen)
    assert all((n_free == 0) == (member.m == member.W) for kb, n_enum, n_free, m in seen)
    return seen


@pytest.mark.parametrize('member', FAMILY, ids=lambda mb: mb.name)
def test_a_member_three_ways(knobs, capfd, member):
    text = member.yaml()
    eng = engine_for(text)
    try:
        for max_t, max_len in CAPS:
            net, space = compile_problem(parse_input_text(text, max_t, Mode.ATTRACT))
            eng.set_problem(net, space)
            capfd.readouterr()
            os.environ['BSX_DEBUG'] = '1'
            try:
                three_ways(eng, member.n, '2', max_t, max_len)
            finally:
                os.environ.pop('BSX_DEBUG', None)
            debug_lines(capfd, member)
    finally:
        eng.close()


@pytest.mark.parametrize('member', WIDE, ids=lambda mb: mb.name)
def test_the_bench_shape_at_two_and_four_state_words(knobs, capfd, member):
    """The m = 6 member padded with single-digit rules to n = 49 (two state words, the whole space) and n = 80 (the
    four-word build, a block of 2^63 problems whose fixed digits belong to layer 0 and change nothing), against the
    per-child level and in closed form: every ring value's basin is the block size / 2^R, summed per necklace."""
    n = member.n
    b = min(n, 63)
    first = 0 if n <= 63 else 0x15A5 << 63
    eng = engine_for(member.yaml())
    try:
        os.environ['BSX_CUBE_DEPTH'] = '2'
        eng.attract2(first, 1 << 30)
        capfd.readouterr()
        os.environ['BSX_DEBUG'] = '1'
        try:
            a = eng.attract2(first, 1 << b)
        finally:
            os.environ.pop('BSX_DEBUG', None)
        debug_lines(capfd, member)
        os.environ['BSX_CUBE_LEAF'] = '0'
        c = eng.attract2(first, 1 << b)
        print('n {}: lower updates per parent {} / per child {}'.format(n, a.stats['lower_executed_steps'], c.stats['lower_executed_steps']))
        assert outcome(a) == outcome(c)
        assert a.stats['lower_executed_steps'] < c.stats['lower_executed_steps']
        table = sorted(record_ints(r) for r in a.table)
        assert sum(r[2] for r in table) + a.n_no_attractor == 1 << b and a.n_no_attractor == 0
        assert sorted((r[1], r[2]) for r in table) == sorted((lam, lam << (b - R)) for lam in necklaces(R).values())
    finally:
        eng.close()
