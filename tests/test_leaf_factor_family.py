"""
CPU proof of what the members of tests/leaf_factor_family.py claim, which tests/test_gpu_leaf_factor.py runs on the GPU: from
the compiled network's wiring and truth tables, by brute force -- kb (the layer-1 digits F^1 depends on and F^2 does not),
the dependent rules, m (the digits some rule reads together with another), and that children hit: for every ring value
the children whose layer-0 update equals that of the all-zero child, which is the cycle state's.
"""
import numpy as np
import pytest

from boolsi_amd.compile import compile_problem
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text
from leaf_factor_family import FAMILY, R, WIDE


def sensitive(tt, k, j):
    return any(((tt >> x) ^ (tt >> (x ^ (1 << j)))) & 1 for x in range(1 << k))


@pytest.mark.parametrize('member', FAMILY + WIDE, ids=lambda mb: mb.name)
def test_the_member_is_what_it_claims(member):
    net, space = compile_problem(parse_input_text(member.yaml(), np.inf, Mode.ATTRACT))
    W, D = member.W, member.D
    assert net.n_nodes == member.n == R + W + D
    preds, masks = net.predecessor_lists, net.tt_masks
    ring, lay1, lay0 = range(R), range(R, R + W), range(R + W, R + W + D)
    # the ring rotates, layer 1 falls to 0, nobody reads layer 0: F^2 depends on the ring alone
    assert all(preds[i] == [(i + 1) % R] and masks[i] == 0b10 for i in ring)
    assert all(masks[i] == 0 for i in lay1)
    assert all(p < R + W for i in range(net.n_nodes) for p in preds[i])
    # kb: every layer-1 digit is one F^1 depends on (some rule's table is sensitive to it)
    felt = {p for i in lay0 for j, p in enumerate(preds[i]) if p in lay1 and sensitive(masks[i], len(preds[i]), j)}
    assert len(felt) == W
    # the dependent rules (wiring): exactly layer 0, of at most four inputs, and m
    reads = {i: {p - R for p in preds[i] if p in lay1} for i in range(net.n_nodes)}
    assert [i for i in range(net.n_nodes) if reads[i]] == list(lay0) and all(len(preds[i]) <= 4 for i in lay0)
    entangled = set().union(*[r for r in reads.values() if len(r) >= 2]) if any(len(r) >= 2 for r in reads.values()) else set()
    assert len(entangled) == member.m
    print('{}: kb {}, {} dependent rules ({} with several added digits), m {}'.format(member.name, W, D, sum(len(r) >= 2 for r in reads.values()), member.m))
    # hits: children (layer-1 assignments) whose layer 0 after one update is what the all-zero child's is
    children = np.arange(1 << W, dtype=np.int64)
    hits = []
    for r in range(1 << R):
        ok = np.ones(len(children), dtype=bool)
        for i in lay0:
            idx = np.zeros(len(children), dtype=np.int64)
            for j, p in enumerate(preds[i]):
                idx |= (((children >> (p - R)) & 1) if p in lay1 else (r >> p) & 1) << j
            table = np.array([(masks[i] >> x) & 1 for x in range(1 << len(preds[i]))], dtype=np.int64)
            v = table[idx]
            ok &= v == v[0]
        hits.append(int(ok.sum()))
    print('hits per ring value: min {} max {} total {}'.format(min(hits), max(hits), sum(hits)))
    assert min(hits) >= 1 and max(hits) > 1 and min(hits) < 1 << W
    if member.name == 'kb10_m0':
        # the digits with two rules: about the value 1 the two contradict for some ring values and agree for others
        seen = set()
        for q in (0, 1, 2):
            two = [i for i in lay0 if reads[i] == {q}]
            assert len(two) == 2
            for r in range(1 << R):
                allows = []
                for i in two:
                    val = lambda a: (masks[i] >> sum(((a if p in lay1 else (r >> p) & 1) << j) for j, p in enumerate(preds[i]))) & 1
                    allows.append(val(1) == val(0))
                seen.add(tuple(allows))
        assert {(True, True), (True, False), (False, True)} <= seen
