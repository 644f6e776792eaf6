"""
Hand-over between the levels of a cube cascade (DESIGN.md "cascade as one chain"): each workgroup of a level reserves a span
of the next level's list on that level's descriptor and copies its segment of listed classes there; the cursor is the
list's length.  Against the CPU oracle: forced depths on the north star with the lower levels on one stream and on the side
streams, segment caps at 1, at the largest segment's count and one below it, and a top level that lists every class it has
(every workgroup of the grid reserves a span).
"""
import os
import re

import numpy as np
import pytest

from boolsi_amd import synth

from test_gpu_cubes import same_as_oracle, setup

pytestmark = pytest.mark.gpu

ENV = ('BSX_CUBES', 'BSX_CUBE_DEPTH', 'BSX_CUBE_NEAR_CAP', 'BSX_CUBE_SPLIT', 'BSX_CUBE_STREAMS', 'BSX_DEBUG')
BASE = 0x0123456789ABCDEF & ~((1 << 28) - 1)


@pytest.fixture()
def eng():
    from boolsi_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()
    for k in ENV:
        os.environ.pop(k, None)


def levels(err):
    """(depth, top?, classes, near a cycle) of every level the library reported (BSX_DEBUG)."""
    return [(int(m.group(1)), m.group(2) is not None, int(m.group(3)), int(m.group(4))) for m in
            re.finditer(r'depth (\d+)( \(top\))?[^,]*, \d+ digits here \(\d+ relevant\), (\d+) classes, (\d+) near a cycle', err)]


@pytest.mark.parametrize('depth', ['3', '5'])
@pytest.mark.parametrize('streams', [None, '1'])
def test_forced_depths_on_the_north_star(eng, depth, streams):
    os.environ['BSX_CUBE_SPLIT'] = '1'                  # several chains: their lower levels share the side streams
    os.environ['BSX_CUBE_DEPTH'] = depth
    if streams:
        os.environ['BSX_CUBE_STREAMS'] = streams
    net, space = setup(eng, synth.north_star_yaml())
    g = same_as_oracle(eng, net, space, BASE, 1 << 24)
    assert g.stats['kernel_launches'] >= 8
    same_as_oracle(eng, net, space, BASE + (1 << 24), 1 << 24)
    same_as_oracle(eng, net, space, BASE + (1 << 25) + 999, (1 << 23) + 12345)


def or_tree_yaml(tree=19, chain=4, idle=2):
    """s <- an OR tree of `tree` nodes (heap order, leaves constant 0), a delay line p -> q1 -> .. -> q_chain nobody reads,
    and `idle` constant nodes nobody reads.  After 5 updates every state is one of the two fixed points (s = OR of the
    initial bits, everything else 0), and F^5 depends on s and the tree alone, while F^1 .. F^4 also read p through the
    delay line: at depth 5 every class of the top level is listed.  (The idle digits make a block of 2^(tree + 4) problems
    two digits wider than what its first update reads, as a cube needs.)"""
    t = ['t{}'.format(i) for i in range(1, tree + 1)]
    q = ['q{}'.format(i) for i in range(1, chain + 1)]
    z = ['z{}'.format(i) for i in range(1, idle + 1)]
    names = ['s'] + t + ['p'] + z + q                   # (s, the tree, p and the idle nodes are the low digits of a problem index)
    rules = dict({'s': 's or t1', 'p': "'0'"}, **{v: "'0'" for v in z})
    for i in range(1, tree + 1):
        kids = [t[c - 1] for c in (2 * i, 2 * i + 1) if c <= tree]
        rules['t{}'.format(i)] = ' or '.join(kids) if kids else "'0'"
    for i in range(1, chain + 1):
        rules['q{}'.format(i)] = 'p' if i == 1 else 'q{}'.format(i - 1)
    lines = ['nodes:'] + ['    - ' + v for v in names] + ['', 'update rules:']
    lines += ['    {}: {}'.format(v, rules[v]) for v in names]
    lines += ['', 'initial state:'] + ['    {}: any'.format(v) for v in names]
    return '\n'.join(lines) + '\n'


def test_segment_caps_around_the_largest_segment(eng, capfd):
    """On or_tree_yaml at depth 5 the top level lists every class, and its classes are shared out evenly over the waves: the
    largest segment's count M is the smallest cap under which nothing overflows (the levels below list far fewer).
    Caps 1 and M - 1 overflow (the chain is redone shallower), M does not; all three against the oracle."""
    os.environ['BSX_CUBE_DEPTH'] = '5'
    os.environ['BSX_CUBE_SPLIT'] = '0'                  # (one chain)
    os.environ['BSX_DEBUG'] = '1'
    text, count = or_tree_yaml(), 1 << 23

    def overflowed(cap):
        os.environ['BSX_CUBE_NEAR_CAP'] = str(cap)
        setup(eng, text, np.inf)                        # (a fresh problem: no depth cap remembered from an overflow)
        capfd.readouterr()
        eng.attract(0, count)
        err = capfd.readouterr().err
        assert any(d == 5 and top for d, top, _, _ in levels(err)), 'no depth-5 chain ran'
        return 'a list overflowed' in err

    hi = 64
    while overflowed(hi):
        hi *= 2
        assert hi <= 1 << 20
    lo = 0                                              # overflowed(lo) or lo == 0, not overflowed(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if mid > 0 and overflowed(mid):
            lo = mid
        else:
            hi = mid
    m = hi
    assert m >= 64
    for cap, over in ((1, True), (m - 1, True), (m, False)):
        os.environ['BSX_CUBE_NEAR_CAP'] = str(cap)
        net, space = setup(eng, text, np.inf)
        capfd.readouterr()
        same_as_oracle(eng, net, space, 0, count, max_t=np.inf)
        assert ('a list overflowed' in capfd.readouterr().err) == over


def test_every_workgroup_reserves_a_span(eng, capfd):
    os.environ['BSX_CUBE_DEPTH'] = '5'
    os.environ['BSX_CUBE_SPLIT'] = '0'
    os.environ['BSX_CUBE_NEAR_CAP'] = str(1 << 14)     # (room for a whole share of the top level per workgroup)
    os.environ['BSX_DEBUG'] = '1'
    net, space = setup(eng, or_tree_yaml(), np.inf)
    capfd.readouterr()
    got = same_as_oracle(eng, net, space, 0, 1 << 23, max_t=np.inf)
    assert len(got.table) == 2
    err = capfd.readouterr().err
    assert 'a list overflowed' not in err
    tops = [lv for lv in levels(err) if lv[1]]
    # 2^20 classes at the top (the tree and s), shared out over every wave of the grid, all of them listed
    assert (5, True, 1 << 20, 1 << 20) in tops
    assert any(d == 4 and not top and classes == 1 << 21 for d, top, classes, _ in levels(err))
