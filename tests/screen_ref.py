"""
TEST INFRASTRUCTURE -- the exact reference of the mutant screens (bsx_run_screen_sampled; include/bsx.h has the
definition), and the cases, sample ranges and mutant lists of its tests (tests/test_screen_ref.py on the CPU,
tests/test_gpu_screen.py and tests/test_gpu_screen_cli.py on the GPU).  Nothing under boolsi_amd/ imports it.

ScreenRef is a WideRef whose problem() also fixes the mutant's nodes (fmask / fval) and leaves the initial state alone:
a listed node keeps its s(0) value at t = 0 and has the mutant's value at every t >= 1, as an origin fixed node does.  A
screen's reference is ScreenRef.attract over sample_ref.sample_indices of the CURRENT space, through wide_ref.aggregate,
and nothing else.  Everything is a pure function of its arguments and computed once per process.
"""
import functools

from boolsi_amd.compile import compile_problem
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text

import sample_ref
from damage_cases import CASES, L_OF, REFUSED, compiled          # noqa: F401  (the tests take them from here)
from sampled_cases import FIRST, SEED, any_case, spread
from wide_ref import WideRef, aggregate

# The fixed-node identity: name -> the arguments of sampled_cases.any_case behind sampled_cases.CASES[name] and the origin's
# fixed nodes; mutants of constant free nodes (single ones with both values, and a double one)
RECIPES = {
    'n300': ((300, 2, 2, spread(300, 40, 3)), {}),
    'n64': ((64, 2, 11, spread(64, 24, 1)), {7: '1'}),
}
CONSTANT_MUTANTS = {
    'n300': [((0, 0),), ((0, 1),), ((150, 0),), ((150, 1),), ((298, 0),), ((298, 1),), ((0, 1), (298, 0))],
    'n64': [((2, 0),), ((2, 1),), ((62, 1),), ((2, 1), (62, 0))],
}


@functools.lru_cache(maxsize=None)
def compiled_with(name, extra_fixed):
    """-> (net, space) of the case with the nodes of `extra_fixed` ((node, value) pairs) listed under `fixed nodes` too"""
    args, fixed = RECIPES[name]
    every = dict(fixed)
    every.update({node: str(value) for node, value in extra_fixed})
    return compile_problem(parse_input_text(any_case(*args, fixed=every or None), 100000, Mode.SIMULATE))


class ScreenRef(WideRef):
    def __init__(self, net, space, mutant):
        super().__init__(net, space)
        self.mutant = tuple(mutant)

    def problem(self, index):
        p = super().problem(index)
        for node, value in self.mutant:
            p.fmask[node], p.fval[node] = True, value
        return p


def count_of(name):
    """G + 37 samples (G = 32 L, a group): with FIRST an unaligned range whose second group is ragged."""
    return 32 * L_OF[name] + 37


@functools.lru_cache(maxsize=None)
def records(name, mutant, first=FIRST, count=None, max_t=None, max_len=None, seed=SEED):
    """Per-sample reference records (found, key, lambda, mu, t_stop) of `mutant` over samples [first, first + count)."""
    net, space, _ = compiled(name)
    count = count_of(name) if count is None else count
    return ScreenRef(net, space, mutant).attract(sample_ref.sample_indices(space, seed, range(first, first + count)), max_t, max_len)[0]


def table_of(name, mutant, **kw):
    """-> ({key: [length, count, sum_l, sum_l2]}, samples without an attractor)"""
    return aggregate(records(name, tuple(mutant), **kw))


def moved_samples(wild, wild_none, table, none):
    """sum over the wild type's keys and the no-attractor bucket of max(0, c_wt - c_m)"""
    return sum(max(0, e[1] - table.get(key, [0, 0])[1]) for key, e in wild.items()) + max(0, wild_none - none)


def node_sets(name):
    """-> (n, 'any' nodes, free constant nodes, nodes the origin fixes)"""
    net, space, _ = compiled(name)
    any_nodes = space.any_nodes.tolist()
    fixed = sorted(int(node) for node, _ in space.fixed.tolist())
    const = [i for i in range(net.n_nodes) if i not in set(any_nodes) and i not in set(fixed)]
    return net.n_nodes, any_nodes, const, fixed


@functools.lru_cache(maxsize=None)
def mutants_of(name):
    """The mutants of a case, the wild type first: the first 'any' node = 0 and the last = 1; the first free constant node
    with both values and the last = 1 (where the case has constant nodes); a double mutant (second 'any' node = 1, node
    n / 2 = 0); node 0 = 0, node n - 1 = 0 and node 256 = 1 (where present); at n600_wide_inputs node 123 (12 predecessors)
    = 1 and its first predecessor = 0."""
    n, any_nodes, const, fixed = node_sets(name)
    out = [(), ((any_nodes[0], 0),), ((any_nodes[-1], 1),)]
    if const:
        out += [((const[0], 0),), ((const[0], 1),), ((const[-1], 1),)]
    assert any_nodes[1] != n // 2
    out.append(((any_nodes[1], 1), (n // 2, 0)))
    out += [((0, 0),), ((n - 1, 0),)]
    if n > 256:
        out.append(((256, 1),))
    if name == 'n600_wide_inputs':
        net = compiled(name)[0]
        preds = net.pred_idx[net.pred_offsets[123]:net.pred_offsets[124]].tolist()
        assert len(preds) == 12
        out += [((123, 1),), ((preds[0], 0),)]
    unique = []
    for m in out:
        assert all(node not in fixed for node, _ in m), (name, m)
        if m not in unique:
            unique.append(m)
    return tuple(unique)


@functools.lru_cache(maxsize=None)
def split_max_t(name):
    """A max_t that splits the wild type's samples: the median of mu + lambda over those that find an attractor, less one
    where that is still at least 1 (so that some are found and some are not whenever the values differ)."""
    ends = sorted(r[3] + r[2] for r in records(name, ()) if r[0])
    return max(1, ends[len(ends) // 2] - 1)


def assert_not_vacuous(name):
    """From the reference alone: two mutants whose tables differ from each other and from the wild type's; a record with
    lambda > 1 and one with mu > 0; under the splitting max_t a mutant with some samples found and some not."""
    tables = [table_of(name, m) for m in mutants_of(name)]
    wild = tables[0]
    others = [t for t in tables[1:] if t != wild]
    assert any(a != b for i, a in enumerate(others) for b in others[i + 1:]), 'no two mutants differ from each other and the wild type'
    recs = [r for m in mutants_of(name) for r in records(name, m) if r[0]]
    assert any(r[2] > 1 for r in recs), 'no cycle longer than 1'
    assert any(r[3] > 0 for r in recs), 'no transient'
    t = split_max_t(name)
    assert any(0 < sum(1 for r in records(name, m, max_t=t) if r[0]) < count_of(name) for m in split_mutants(name)), 'the cap does not split'


def split_mutants(name):
    """The mutants run under the splitting max_t: the wild type and the double mutant."""
    ms = mutants_of(name)
    return (ms[0], next(m for m in ms if len(m) == 2))
