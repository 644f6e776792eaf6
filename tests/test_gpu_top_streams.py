"""
BSX_CUBE_TOP_STREAMS=2 (DESIGN.md "Tops on two streams"): the top levels of a batch's consecutive chains alternate between
the handle's stream and a second one, so that a top's workgroups take the CUs the previous top's free.  Only the order of
launches changes, so: identical table, no-attractor count and reference steps with one top stream and with two -- where
slots of list buffers are reused (more listing chains than side streams), without side streams (the second stream stays
unused), on a fresh handle's first call (the mirror image is rebuilt between two batches) and with segments so small
that chains restart shallower.
"""
import os

import pytest

from boolsi_amd import synth
from boolsi_amd.attract import merge_tables
from boolsi_amd.compile import compile_problem
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text

pytestmark = pytest.mark.gpu
KNOBS = ('BSX_CUBE_TOP_STREAMS', 'BSX_CUBE_SPLIT', 'BSX_CUBE_STREAMS', 'BSX_CUBE_NEAR_CAP')
MAX_T = 4096
FIRST, COUNT = 0x0123456789ABCDEF & ~((1 << 56) - 1), 1 << 56       # a north-star block of 2^56 at a fixed offset


@pytest.fixture()
def knobs():
    yield
    for k in KNOBS:
        os.environ.pop(k, None)


def fresh_engine():
    from boolsi_amd.engine import Engine
    net, space = compile_problem(parse_input_text(synth.north_star_yaml(), MAX_T, Mode.ATTRACT))
    eng = Engine(0)
    eng.set_problem(net, space)
    return eng


def outcome(r):
    return merge_tables([r.table]), r.n_no_attractor, r.stats['state_steps']


def run(eng, top_streams, count=COUNT, **env):
    os.environ['BSX_CUBE_TOP_STREAMS'] = top_streams
    os.environ.update(env)
    try:
        return eng.attract2(FIRST, count, MAX_T)
    finally:
        for k in ('BSX_CUBE_TOP_STREAMS',) + tuple(env):
            os.environ.pop(k)


@pytest.fixture(scope='module')
def unsplit():
    """The block as one cube, one top stream: what every split run below must give."""
    eng = fresh_engine()
    try:
        eng.attract2(FIRST, COUNT, MAX_T)               # (first contact with the attractors)
        r = run(eng, '1', BSX_CUBE_SPLIT='0')
        assert sum(v[1] for v in merge_tables([r.table]).values()) + r.n_no_attractor == COUNT
        return outcome(r)
    finally:
        eng.close()


@pytest.mark.parametrize('side_streams', [None, '2', '1'])
def test_split_block_with_one_and_two_top_streams(knobs, unsplit, side_streams):
    """BSX_CUBE_SPLIT=1: an eight-leaf tree, more listing chains than side streams (four by default, two here), so slots of
    list buffers are reused behind their events; BSX_CUBE_STREAMS=1: no side streams, both settings run on one stream."""
    env = {'BSX_CUBE_SPLIT': '1'}
    if side_streams:
        env['BSX_CUBE_STREAMS'] = side_streams
    eng = fresh_engine()
    try:
        eng.attract2(FIRST, COUNT, MAX_T)
        one = run(eng, '1', **env)
        two = run(eng, '2', **env)
        again = run(eng, '2', **env)
        # (more than eight launches: the block was split; their number varies from call to call with what the handle has seen)
        assert min(r.stats['kernel_launches'] for r in (one, two, again)) > 8
        assert outcome(one) == outcome(two) == outcome(again) == unsplit
    finally:
        eng.close()


def test_first_call_on_a_fresh_handle(knobs, unsplit):
    """Nothing cached: discovery, then batches between which the journal grows and the image is rebuilt."""
    eng = fresh_engine()
    try:
        assert outcome(run(eng, '2', BSX_CUBE_SPLIT='1')) == unsplit
    finally:
        eng.close()


def test_tiny_segments_restart_chains_shallower(knobs):
    """Segments of seven classes: lists overflow and chains are redone from a shallower top, down to depth 1 -- on a block
    of 2^32, which is quick even then.  A handle remembers the depth cap of a restart, so each setting gets a fresh one."""
    got = []
    for top_streams, env in (('1', {'BSX_CUBE_SPLIT': '0'}), ('1', {'BSX_CUBE_SPLIT': '1', 'BSX_CUBE_NEAR_CAP': '7'}),
                             ('2', {'BSX_CUBE_SPLIT': '1', 'BSX_CUBE_NEAR_CAP': '7'})):
        eng = fresh_engine()
        try:
            eng.attract2(FIRST, 1 << 32, MAX_T)
            got.append(outcome(run(eng, top_streams, 1 << 32, **env)))
        finally:
            eng.close()
    assert got[0] == got[1] == got[2]
