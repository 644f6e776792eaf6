"""
The damage-spreading reference itself (tests/damage_ref.py, no GPU): closed forms on networks whose damage is known, and
the non-vacuity of the cases the GPU tests compare with it (tests/damage_cases.py).
"""
import numpy as np
import pytest

from boolsi_amd.compile import compile_problem
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text

import damage_cases
import damage_ref
from test_gpu_wide_exact import yaml_of
from wide_ref import WideRef

SEED, FIRST, COUNT, T = 7, 1000003, 101, 6


def reference(preds, masks, init, fixed=None):
    net, space = compile_problem(parse_input_text(yaml_of(preds, masks, init, fixed=fixed), 100000, Mode.SIMULATE))
    return WideRef(net, space)


@pytest.mark.parametrize('h', [1, 3, 40])
def test_identity_network_keeps_the_distance(h):
    n = 40
    ref = reference([[i] for i in range(n)], [0b10] * n, ['any' if i % 3 else '1' for i in range(n)])
    d = damage_ref.distances(ref, SEED, FIRST, COUNT, h, T)
    assert np.array_equal(d, np.full((T + 1, COUNT), h))


def test_rotation_moves_the_damage_and_keeps_its_size():
    n = 40
    ref = reference([[(i + 1) % n] for i in range(n)], [0b10] * n, ['any'] * n)
    assert np.array_equal(damage_ref.distances(ref, SEED, FIRST, COUNT, 5, T), np.full((T + 1, COUNT), 5))


@pytest.mark.parametrize('h', [1, 7])
def test_constant_network_merges_after_one_step(h):
    n = 40
    ref = reference([[i] for i in range(n)], [0b11 if i % 2 else 0b00 for i in range(n)], ['any'] * n)
    d = damage_ref.distances(ref, SEED, FIRST, COUNT, h, T)
    assert np.array_equal(d[0], np.full(COUNT, h)) and not d[1:].any()
    assert damage_ref.sums(d, n)[2] == [0] + [COUNT] * T


def test_a_fixed_node_is_never_flipped():
    n = 12
    fixed = {2: '1', 7: '0'}
    ref = reference([[i] for i in range(n)], [0b10] * n, ['any'] * n, fixed=fixed)
    free = damage_ref.free_nodes(ref)
    assert free == [i for i in range(n) if i not in fixed]
    X, Y = damage_ref.pairs(ref, SEED, range(FIRST, FIRST + 400), 1)
    flipped = (X ^ Y).sum(axis=0)
    assert flipped.sum() == 400 and not flipped[2] and not flipped[7]
    assert all(flipped[i] > 0 for i in free)
    # all free nodes at once: exactly the free nodes differ, and the fixed nodes take their value from t = 1 on
    X, Y = damage_ref.pairs(ref, SEED, range(FIRST, FIRST + 9), len(free))
    assert (X ^ Y).sum(axis=0).tolist() == [0 if i in fixed else 9 for i in range(n)]
    d = damage_ref.distances(ref, SEED, FIRST, 9, len(free), 3)
    assert np.array_equal(d, np.full((4, 9), len(free)))


def test_sums_fold_the_distances():
    d = np.array([[2, 2, 2], [0, 5, 1]])
    assert damage_ref.sums(d, 5) == ([6, 6], [12, 26], [0, 1], [[0, 0, 3, 0, 0, 0], [1, 1, 0, 0, 0, 1]])


def test_the_example_of_the_definition():
    """n1024, one flip: figures worked out once by hand-run of the definition, kept as a pin of the reference."""
    sum_d, _, merged, _ = damage_cases.expect('n1024', 1)
    d = damage_cases.distances('n1024', 1)
    assert [(sum_d[t], merged[t], int(d[t].max())) for t in (0, 1, 12)] == [(293, 0, 1), (279, 109, 4), (342, 254, 28)]


@pytest.mark.parametrize('name', list(damage_cases.CASES))
def test_cases_are_not_vacuous(name):
    for h in damage_cases.FLIPS:
        damage_cases.expect(name, h)        # asserts
    for refused in damage_cases.REFUSED:
        sp = damage_cases.compiled(refused)[1]
        assert len(sp.fixed_var) or len(sp.pert_var) or len(sp.sched)
