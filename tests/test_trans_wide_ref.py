"""
tests/trans_wide_ref.py (the reference of the attractor transitions above 256 nodes, on tests/wide_ref.py's stepping)
against tests/trans_ref.py (the CPU oracle's step, pinned to the oracle's attract by tests/test_trans_ref.py), on
networks of at most 256 nodes where both exist.  No GPU.  Edges, node_exits and the detail counters must be equal without
a cap and under caps that leave flips unresolved; flip by flip, (resolved, mu, lambda', key, row) must be equal; and the
refusals of a table (an open row, a duplicate, a length that is a multiple of the period) must be the same assertions.
"""
import os

import numpy as np
import pytest

import trans_ref
import trans_wide_ref
from test_gpu_profile import WIDTH_CASES, compiled, oracle_table, random_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE2 = os.path.join(ROOT, 'tests', 'golden', 'examples', 'output3_example2', 'example2.yaml')
INF = float('inf')


def example2_case():
    _, net, space = compiled(open(EXAMPLE2).read())
    return net, space, oracle_table(net, space, 8)


def width_case(name):
    n, seed, fixed, many = WIDTH_CASES[name]
    _, net, space = compiled(random_text(n, seed, fixed=fixed, many_preds=many))
    return net, space, oracle_table(net, space, 1 << 10)


CASES = {'example2': (example2_case, (INF, 4, 1, 0)),
         'n64_fixed': (lambda: width_case('n64_fixed'), (INF, 8, 0)),
         'n64_capped': (lambda: width_case('n64'), (19, 18, 5)),
         'n100_many_preds': (lambda: width_case('n100_many_preds'), (INF, 14))}


@pytest.mark.parametrize('name', sorted(CASES))
def test_equals_trans_ref(name):
    make, caps = CASES[name]
    net, space, table = make()
    keys = sorted(table)
    lengths = [table[k] for k in keys]
    old = trans_ref.TransRef(net, space, keys, lengths)
    new = trans_wide_ref.TransWideRef(net, space, keys, lengths)
    assert new.free == old.free and new.rows == old.rows and new.listed == old.listed
    if name == 'n64_fixed':
        assert len(new.free) == 62                                      # guard: fixed nodes
    unresolved = []
    for max_t in caps:
        want_edges, want_exits, want_detail = old.transitions(max_t)
        edges, exits, detail = new.transitions(max_t)
        assert edges == want_edges and np.array_equal(exits, want_exits)
        assert {k: detail[k] for k in want_detail} == want_detail
        unresolved.append(detail['unresolved'])
        for q, j, i, x0 in old.flips():
            assert new.flip_outcome(x0, max_t) == old.flip_outcome(x0, max_t), (max_t, q, j, i)
    assert list(new.flips()) == list(old.flips())
    if name in ('example2', 'n64_capped'):
        assert any(unresolved) and len(set(unresolved)) > 1             # guard: a capped run with unresolved flips


def test_refusals_are_trans_refs():
    net, space, table = width_case('n64')
    keys = sorted(table)
    lengths = [table[k] for k in keys]
    assert lengths == [4, 4]                                            # guard: what the cases below are built on
    bad = {'open': (keys, [4, 3], 'row 1 is not closed'),
           'duplicate': (keys + keys[:1], lengths + lengths[:1], 'row 2 shares a state'),
           'multiple': (keys, [4, 8], 'row 1 shares a state')}
    for name, (k, l, text) in bad.items():
        for cls in (trans_ref.TransRef, trans_wide_ref.TransWideRef):
            with pytest.raises(AssertionError) as err:
                cls(net, space, k, l)
            assert text in str(err.value), (name, cls.__name__)


def test_a_row_may_start_anywhere_on_its_cycle():
    """the canonical key of a row is its minimum state, whatever state the row is listed from"""
    net, space, table = width_case('n64')
    keys = sorted(table)
    ref = trans_wide_ref.TransWideRef(net, space, keys, [table[k] for k in keys])
    moved = trans_wide_ref.TransWideRef(net, space, [ref.rows[0][2], keys[1]], ref.lengths)
    assert moved.rows[0] == ref.rows[0][2:] + ref.rows[0][:2] and moved.keys[0] != keys[0]
    edges, exits, _ = ref.transitions()
    edges2, exits2, _ = moved.transitions()
    assert edges2 == edges and int(exits2.sum()) == int(exits.sum())
    assert moved.flip_outcome(ref.rows[0][1] ^ 1)[3:] == ref.flip_outcome(ref.rows[0][1] ^ 1)[3:]
