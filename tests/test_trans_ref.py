"""
tests/trans_ref.py, the dict-based reference of the attractor transitions, against the CPU oracle's own attract (no
GPU).  For every flip x_0 of example2 and of WIDTH_CASES['n20'] a problem space is built whose origin state is x_0
(no 'any' nodes, the origin's fixed nodes, nothing else): Oracle.attract(0, 1, max_t) must report the same found / key /
length / trajectory length (= mu, the last perturbation time being 0) as TransRef.flip_outcome.  Run without a cap and
at two finite caps that split the flips into resolved and unresolved ones.
"""
import dataclasses
import os

import numpy as np
import pytest

from boolsi_amd.compile import code_to_words

import trans_ref
from test_gpu_profile import WIDTH_CASES, compiled, oracle_table, random_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE2 = os.path.join(ROOT, 'tests', 'golden', 'examples', 'output3_example2', 'example2.yaml')
INF = float('inf')


def example2_case():
    _, net, space = compiled(open(EXAMPLE2).read())
    return net, space, oracle_table(net, space, 8)


def n20_case():
    n, seed, fixed, many = WIDTH_CASES['n20']
    _, net, space = compiled(random_text(n, seed, fixed=fixed, many_preds=many))
    return net, space, oracle_table(net, space, 1 << 10)


CASES = {'example2': (example2_case, (INF, 3, 1)), 'n20': (n20_case, (INF, 28, 4))}


def space_at(space, net, x0):
    return dataclasses.replace(space, origin_state=code_to_words(x0, net.n_words), any_nodes=np.zeros(0, np.uint32),
                               n_problems=1, radices=[])


@pytest.mark.parametrize('name', sorted(CASES))
def test_flip_outcomes_are_the_oracles(name):
    from oracle.cpu_oracle import Oracle, key_int
    make, caps = CASES[name]
    net, space, table = make()
    assert len(space.fixed_var) == 0 and len(space.sched) == 0 and len(space.pert_var) == 0
    keys = sorted(table)
    ref = trans_ref.TransRef(net, space, keys, [table[k] for k in keys])
    flips = list(ref.flips())
    assert len(flips) == sum(table.values()) * net.n_nodes
    for max_t in caps:
        found = 0
        for q, j, i, x0 in flips:
            resolved, mu, lam, key, _ = ref.flip_outcome(x0, max_t)
            pp, tab, none, _ = Oracle(net, space_at(space, net, x0)).attract(0, 1, max_t)
            assert bool(pp[0]['found']) == resolved and none == (0 if resolved else 1), (max_t, q, j, i)
            if resolved:
                assert (key_int(pp[0]['key']), int(pp[0]['length']), int(pp[0]['trajectory_l'])) == (key, lam, mu), (max_t, q, j, i)
                found += 1
        if max_t == INF:
            assert found == len(flips)
        else:
            assert 0 < found < len(flips), (max_t, found)             # guard: the cap splits the flips


def test_example2_shape():
    """what the issue states about the smallest case: 2 attractors of lengths 1 and 3, 12 flips, 3 edges, 2 of them cross"""
    net, space, table = example2_case()
    keys = sorted(table)
    lengths = [table[k] for k in keys]
    assert sorted(lengths) == [1, 3]
    ref = trans_ref.TransRef(net, space, keys, lengths)
    edges, exits, detail = ref.transitions()
    assert sum(e[2] for e in edges) == 12 and len(edges) == 3 and len(trans_ref.cross_edges(edges)) == 2
    for q, length in enumerate(lengths):
        assert sum(e[2] for e in edges if e[0] == q) == length * 3
        assert int(exits[q].sum()) == sum(e[2] for e in edges if e[0] == q and e[1] != q)
    assert detail['outside'] == 0 and detail['unresolved'] == 0
    # a cap of 0 resolves nothing
    edges0, _, _ = ref.transitions(0)
    assert [(e[1], e[3]) for e in edges0] == [(trans_ref.UNRESOLVED, 0)] * 2
