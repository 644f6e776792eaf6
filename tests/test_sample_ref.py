"""
tests/sample_ref.py against tests/wide_ref.py (no GPU): the flat index I(j) of a sample decodes, through
WideRef.problem, to the state bits and the variation choices that the sample drew; the indices of adjacent sample
ranges concatenate; the numpy generator words equal the Python-int ones.
"""
import numpy as np
import pytest

import sample_ref
from sampled_cases import FIRST, SEED, compiled
from wide_ref import digit_state

SAMPLES = [0, 1, 63, 64, 65, FIRST, FIRST + 61, 2 ** 32 + 17, 2 ** 64 - 1]


@pytest.mark.parametrize('name', ['n20', 'example2', 'n300', 'n700_variations'])
def test_flat_index_decodes_to_what_the_sample_drew(name):
    net, space, ref = compiled(name)
    n_any, V = len(space.any_nodes), sample_ref.variant_count(space)
    assert V << n_any == space.n_problems
    variants = set()
    for j, index in zip(SAMPLES, sample_ref.sample_indices(space, SEED, SAMPLES)):
        bits, variant = sample_ref.sample(SEED, j, n_any, V)
        assert 0 <= variant < V and index == sum(b << a for a, b in enumerate(bits)) + (variant << n_any)
        variants.add(variant)
        prob = ref.problem(index)
        want = ref.origin.copy()
        want[space.any_nodes] = bits
        assert np.array_equal(prob.init, want)
        # the variation choices: digits of the variant number, fixed-node variations first, least significant first
        v = variant
        fmask = {node: value for node, value in space.fixed.tolist()}
        for node, rc in space.fixed_var.tolist():
            radix = 3 if rc == 3 else 2
            s = digit_state(rc, v % radix)
            v //= radix
            if s is not None:
                fmask[node] = s
        assert {int(i): int(prob.fval[i]) for i in np.flatnonzero(prob.fmask)} == fmask
        pert = {}
        for t, node, value in space.sched.tolist():
            pert.setdefault(t, {})[node] = value
        for t, node, rc in space.pert_var.tolist():
            radix = 3 if rc == 3 else 2
            s = digit_state(rc, v % radix)
            v //= radix
            if s is not None:
                pert.setdefault(t, {})[node] = s
        assert v == 0 and prob.pert == pert
    if V > 1:
        assert len(variants) >= 2


def test_adjacent_ranges_concatenate():
    _, space, _ = compiled('n700_variations')
    a, b, c = FIRST, FIRST + 37, FIRST + 150
    idx = lambda lo, hi: sample_ref.sample_indices(space, SEED, range(lo, hi))        # noqa: E731
    assert idx(a, b) + idx(b, c) == idx(a, c)
    assert idx(a, c) != sample_ref.sample_indices(space, SEED + 1, range(a, c))


def test_numpy_words_equal_the_python_ones():
    for seed in (0, 7, 2 ** 63):
        words = sample_ref.any_words_np(seed, 3, 5, 15624)
        assert words.tolist() == [[sample_ref.any_word(seed, 15624 + b, a) for a in range(5)] for b in range(3)]
