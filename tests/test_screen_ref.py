"""
The reference of the mutant screens (tests/screen_ref.py) against what the project already pins, on the CPU:
  * its wild type is the sampled attract reference (sampled_cases.records);
  * a mutant whose nodes all have a constant initial state gives the records of the plain reference on the space that
    lists those nodes under `fixed nodes` -- the identity the definition of include/bsx.h is built on (s(0) is left alone:
    forcing it would break the identity);
  * moved_samples is an integer, and 0 for the wild type.
"""
import pytest

import sample_ref
import sampled_cases
import screen_ref
from sampled_cases import FIRST, SEED, any_case
from screen_ref import CONSTANT_MUTANTS as MUTANTS, RECIPES, ScreenRef, compiled_with, count_of, mutants_of, table_of
from wide_ref import WideRef, aggregate

@pytest.mark.parametrize('name', ['n64', 'n300'])
def test_the_recipe_is_the_case(name):
    assert any_case(*RECIPES[name][0], fixed=RECIPES[name][1] or None) == sampled_cases.CASES[name]()


@pytest.mark.parametrize('name', ['n64', 'n300'])
def test_the_wild_type_is_the_sampled_reference(name):
    count = count_of(name)
    assert mutants_of(name)[0] == ()
    assert screen_ref.records(name, ()) == sampled_cases.records(name, FIRST, count)
    sampled_cases.assert_not_vacuous(screen_ref.records(name, ()))


@pytest.mark.parametrize('name,mutant', [(name, m) for name in MUTANTS for m in MUTANTS[name]])
def test_constant_node_mutants_equal_the_space_that_fixes_them(name, mutant):
    net, space, _ = screen_ref.compiled(name)
    any_nodes = set(space.any_nodes.tolist())
    assert all(node not in any_nodes for node, _ in mutant)
    count = count_of(name)
    idx = sample_ref.sample_indices(space, SEED, range(FIRST, FIRST + count))
    net2, space2 = compiled_with(name, mutant)
    # the fixed space keeps the 'any' list, so the samples are the same problems
    assert space2.any_nodes.tolist() == space.any_nodes.tolist()
    assert sample_ref.sample_indices(space2, SEED, range(FIRST, FIRST + count)) == idx
    want = aggregate(WideRef(net2, space2).attract(idx)[0])
    assert aggregate(ScreenRef(net, space, mutant).attract(idx)[0]) == want
    assert len(want[0]) >= 1 and want[1] == 0


def test_forcing_the_initial_state_would_break_the_identity():
    """n300, node 0 = 0: the origin has node 0 at 1, and a reference that also forced s(0) gives other records."""
    name, mutant = 'n300', ((0, 0),)
    net, space, _ = screen_ref.compiled(name)

    class Forced(ScreenRef):
        def problem(self, index):
            p = super().problem(index)
            for node, value in self.mutant:
                p.init[node] = value
            return p
    idx = sample_ref.sample_indices(space, SEED, range(FIRST, FIRST + count_of(name)))
    assert (int(space.origin_state[0]) & 1) == 1
    assert aggregate(Forced(net, space, mutant).attract(idx)[0]) != table_of(name, mutant)


@pytest.mark.parametrize('name', ['n64', 'n300'])
def test_moved_samples_is_an_integer_and_zero_for_the_wild_type(name):
    wild, wild_none = table_of(name, ())
    assert screen_ref.moved_samples(wild, wild_none, wild, wild_none) == 0
    moved = [screen_ref.moved_samples(wild, wild_none, *table_of(name, m)) for m in mutants_of(name)]
    assert all(isinstance(v, int) and 0 <= v <= count_of(name) for v in moved)
    assert moved[0] == 0 and any(v > 0 for v in moved)
    # a mutant whose table is the wild type's has moved nothing
    same = [m for m in mutants_of(name)[1:] if table_of(name, m) == (wild, wild_none)]
    assert same and all(moved[mutants_of(name).index(m)] == 0 for m in same)
