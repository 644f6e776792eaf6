"""
The node-influence reference (tests/influence_ref.py, the definition of include/bsx.h restated) against damage_ref where
both apply and against closed forms, without a GPU; then that every case of influence_cases is not vacuous.
"""
import numpy as np
import pytest

from boolsi_amd.compile import compile_problem
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text

import damage_ref
import influence_cases
import influence_ref
import sample_ref
from influence_cases import CASES, FIRST, SEED, T, compiled, count_of, expect, sources_of
from test_gpu_wide_exact import yaml_of
from wide_ref import WideRef


def reference_of(text):
    net, space = compile_problem(parse_input_text(text, 100000, Mode.SIMULATE))
    return WideRef(net, space)


@pytest.mark.parametrize('name', ['n64', 'n300', 'n600_wide_inputs'])
def test_row_sums_are_the_distances_of_explicitly_flipped_states(name):
    """Sum over the targets of influence[s][t] = sum over the samples of popcount D_j(t), recomputed from damage_ref.step on
    states with the source flipped by hand; the merged count likewise."""
    ref = compiled(name)[2]
    count, sources = 100, sources_of(name)[:6]
    influence, merged = influence_ref.counts(ref, SEED, FIRST, count, sources, T)
    X0 = damage_ref.pairs(ref, SEED, range(FIRST, FIRST + count), 0)[0]
    for s, v in enumerate(sources):
        X, Y = X0.copy(), X0.copy()
        for q in range(count):
            Y[q, v] = 1 - Y[q, v]
        for t in range(1, T + 1):
            X, Y = damage_ref.step(ref, X), damage_ref.step(ref, Y)
            d = (X != Y).sum(axis=1)
            assert int(influence[s, t - 1].sum()) == int(d.sum())
            assert int(merged[s, t - 1]) == int((d == 0).sum())


def test_one_flip_of_damage_is_a_mixture_of_the_sources():
    """damage with h = 1 inverts free[p] of sample j; the influence rows of those sources, taken sample by sample, carry the
    same distances."""
    name = 'n64'
    ref = compiled(name)[2]
    count, steps = 64, 6
    free = damage_ref.free_nodes(ref)
    d = damage_ref.distances(ref, SEED, FIRST, count, 1, steps)
    n_any = len(ref.space.any_nodes)
    for q in range(count):
        v = free[damage_ref.positions(SEED, FIRST + q, n_any, len(free), 1)[0]]
        influence, merged = influence_ref.counts(ref, SEED, FIRST + q, 1, [v], steps)
        assert influence.sum(axis=2)[0].tolist() == d[1:, q].tolist()
        assert merged[0].tolist() == [int(x == 0) for x in d[1:, q]]


def test_a_ring_of_copies_moves_the_flip_one_node_per_step():
    n, count, steps = 300, 70, 9
    ref = reference_of(yaml_of([[(i - 1) % n] for i in range(n)], [0b10] * n, ['any'] * n))
    sources = [0, 150, 296, 299]
    influence, merged = influence_ref.counts(ref, SEED, FIRST, count, sources, steps)
    want = np.zeros_like(influence)
    for s, v in enumerate(sources):
        for t in range(1, steps + 1):
            want[s, t - 1, (v + t) % n] = count
    assert np.array_equal(influence, want) and not merged.any()


def test_an_and_gate_passes_a_flip_where_its_other_input_is_on():
    """x_i <- x_{i-1} AND x_{i-2}: the t = 1 count of source i - 1 at target i is the number of samples with x_{i-2} = 1,
    taken from sample_ref."""
    n, count = 64, 200
    ref = reference_of(yaml_of([[(i - 1) % n, (i - 2) % n] for i in range(n)], [0b1000] * n, ['any'] * n))
    sources = [0, 5, 62, 63]
    influence, _ = influence_ref.counts(ref, SEED, FIRST, count, sources, 1)
    for s, v in enumerate(sources):
        i, other = (v + 1) % n, (v - 1) % n     # node i reads v = i - 1 and other = i - 2; 'any' ordinal a = the node itself
        on = sum((sample_ref.any_word(SEED, j >> 6, other) >> (j & 63)) & 1 for j in range(FIRST, FIRST + count))
        assert 0 < on < count and int(influence[s, 0, i]) == on
        # node v + 2 reads v as its i - 2 input: it passes where x_{v+1} is on
        on2 = sum((sample_ref.any_word(SEED, j >> 6, (v + 1) % n) >> (j & 63)) & 1 for j in range(FIRST, FIRST + count))
        assert int(influence[s, 0, (v + 2) % n]) == on2
        assert int(influence[s, 0].sum()) == on + on2


@pytest.mark.parametrize('name', list(CASES))
def test_cases_are_not_vacuous(name):
    influence, merged = expect(name)
    assert influence.shape == (len(sources_of(name)), T, compiled(name)[0].n_nodes) and merged.shape == influence.shape[:2]
    free = damage_ref.free_nodes(compiled(name)[2])
    assert set(sources_of(name)) <= set(free) and len(set(sources_of(name))) == len(sources_of(name))
    if name == 'n64':
        assert list(sources_of(name)) == free
    else:
        assert set(free[:8]) | set(free[-4:]) | set(free[255:259]) <= set(sources_of(name))
    # a merged sample differs nowhere: the counts of a row are bounded by the samples that have not merged
    assert (influence.max(axis=2) <= count_of(name) - merged).all()


def test_disjoint_ranges_add_up_in_the_reference():
    name, cut = 'n300', 101
    whole = expect(name)
    a = influence_cases.counts(name, count=cut)
    b = influence_cases.counts(name, first=FIRST + cut, count=count_of(name) - cut)
    assert np.array_equal(a[0] + b[0], whole[0]) and np.array_equal(a[1] + b[1], whole[1])
