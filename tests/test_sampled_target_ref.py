"""
The cases of the sampled target tests are not vacuous (sampled_target_cases.expect_target: from the reference alone), and
the host layers' flat-index helper (boolsi_amd.engine.flat_indices, which rebuilds a sample's problem index from what
bsx_sample_problems returns) agrees with the definition restated in sample_ref.  No GPU.
"""
import numpy as np
import pytest

import sample_ref
from sampled_cases import FIRST, SEED, compiled
from sampled_target_cases import GENEROUS, INF, TARGETS, brent_stop, count_of, expect_target
from wide_ref import code_of, words_of


@pytest.mark.parametrize('name', list(TARGETS))
def test_target_cases_are_not_vacuous(name):
    out = expect_target(name)
    split = TARGETS[name][2]
    assert len(out[split][0]) < len(out[INF][0]) and out[GENEROUS][0] == out[INF][0]
    # a miss at max_t = inf is a closed cycle: its search ends later than any cap-free hit could tell, never earlier
    assert out[INF][1] >= sum(t for _, t in out[INF][0])


def test_brent_stop():
    # checkpoints at T_max + 0, 1, 3, 7, ...; kept for 1, 2, 4, 8, ... steps
    assert brent_stop(0, 0, 1) == 1
    assert brent_stop(0, 0, 2) == 3             # checkpoint 1 (window 2)
    assert brent_stop(0, 2, 1) == 4             # first checkpoint on the cycle is 3
    assert brent_stop(9, 3, 3) == 9 + 3 + 3     # checkpoint T_max + 3 is the first kept for at least 3 steps
    assert brent_stop(0, 100, 5) == 127 + 5


SCATTERED = [0, 1, 31, 63, 64, 65, FIRST, FIRST + 61, 2 ** 32 + 17, 2 ** 63, 2 ** 64 - 2, 2 ** 64 - 1, 5]


@pytest.mark.parametrize('name', ['n64', 'n577', 'n1024', 'n700_variations'])
def test_flat_index_helper_equals_the_definition(name):
    from boolsi_amd.engine import flat_indices
    net, space, ref = compiled(name)
    n_any, V = len(space.any_nodes), sample_ref.variant_count(space)
    want = [sample_ref.flat_index(SEED, j, n_any, V) for j in SCATTERED]
    # what bsx_sample_problems returns for these samples, built from the definition: s(0) as words, the variant number
    states = np.array([words_of(code_of(ref.problem(i).init), net.n_words) for i in want], np.uint64)
    variants = np.array([i >> n_any for i in want], np.uint64)
    assert flat_indices(states, variants, space.any_nodes) == want
    assert len(set(want)) == len(SCATTERED)
    if V > 1:
        assert len({i >> n_any for i in want}) >= 2
    assert flat_indices(np.zeros((0, net.n_words), np.uint64), np.zeros(0, np.uint64), space.any_nodes) == []
