"""
TEST INFRASTRUCTURE -- networks, sample ranges, source lists and reference results of the node-influence tests
(tests/test_influence_ref.py on the CPU, tests/test_gpu_influence.py and tests/test_gpu_influence_cli.py on the GPU).
Everything is a pure function of its arguments; the reference of a call is influence_ref.counts over the definition and
nothing else.

A range is G + 37 samples from 1000003 (G = 32 L, a group): unaligned, with a ragged second group.  Sources: every free node
at n64; elsewhere the first eight free nodes, the free nodes at positions 255 .. 258 (where there are that many), the last
four, and at n600_wide_inputs one predecessor each of nodes 123 and 300 (the per-trajectory table path of the kernels).
"""
import functools

import damage_cases
import damage_ref
import influence_ref
from damage_cases import L_OF, compiled, count_of
from sampled_cases import FIRST, SEED

T = 12
NAMES = ('n64', 'n257', 'n300', 'n577', 'n1024', 'n600_wide_inputs')
CASES = {name: damage_cases.CASES[name] for name in NAMES}
WIDE_TARGETS = (123, 300)


def wide_predecessors(name):
    """The highest free predecessor of each of the nodes with more than 6 inputs of n600_wide_inputs."""
    net, _, ref = compiled(name)
    free = set(damage_ref.free_nodes(ref))
    return [max(p for p in net.predecessor_lists[node] if p in free and p != node) for node in WIDE_TARGETS]


@functools.lru_cache(maxsize=None)
def sources_of(name):
    free = damage_ref.free_nodes(compiled(name)[2])
    if name == 'n64':
        return tuple(free)
    chosen = set(free[:8]) | set(free[255:259]) | set(free[-4:])
    if name == 'n600_wide_inputs':
        chosen |= set(wide_predecessors(name))
    return tuple(sorted(chosen))


@functools.lru_cache(maxsize=None)
def counts(name, first=FIRST, count=None, steps=T, seed=SEED, sources=None):
    """-> (influence, n_merged) of influence_ref.counts, read-only"""
    got = influence_ref.counts(compiled(name)[2], seed, first, count_of(name) if count is None else count,
                               sources_of(name) if sources is None else sources, steps)
    for a in got:
        a.setflags(write=False)
    return got


@functools.lru_cache(maxsize=None)
def expect(name):
    """-> (influence int64[n_sources, T, n], n_merged int64[n_sources, T]) of samples [FIRST, FIRST + count_of(name)), from the
    reference alone, with the assertions that the case is not vacuous."""
    sources, N = sources_of(name), count_of(name)
    influence, merged = counts(name)
    assert 0 <= influence.min() and influence.max() <= N and 0 <= merged.min() and merged.max() <= N
    partial = (influence > 0) & (influence < N)
    for s, v in enumerate(sources):
        partial[s, :, v] = False
    assert partial.any(), 'no cell with 0 < count < N at a target other than the source'
    assert ((merged[:, T - 1] > 0) & (merged[:, T - 1] < N)).any(), 'at t = T no source has some pairs merged and some not'
    assert (merged[:, 0] == N).any(), 'no source dies at t = 1'
    if name == 'n600_wide_inputs':
        for node, pred in zip(WIDE_TARGETS, wide_predecessors(name)):
            assert influence[sources.index(pred), 0, node] > 0, 'node {} does not feel its predecessor {}'.format(node, pred)
    return influence, merged
