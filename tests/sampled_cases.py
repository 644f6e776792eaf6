"""
TEST INFRASTRUCTURE -- networks, problem spaces and reference results of the sampled attract tests
(tests/test_sample_ref.py on the CPU, tests/test_gpu_sampled.py on the GPU).  Everything is a pure function of its
arguments; the reference of a sampled call is WideRef.attract over sample_ref.sample_indices and nothing else.
"""
import functools
import os
import random

from boolsi_amd import synth
from boolsi_amd.compile import compile_problem
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text

import sample_ref
from test_gpu_wide_exact import many_preds_case, network, yaml_of
from wide_ref import WideRef, aggregate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE2 = os.path.join(ROOT, 'tests', 'golden', 'examples', 'output3_example2', 'example2.yaml')
SEED = 7
FIRST = 1000003             # unaligned: 1000003 = 64 * 15625 + 3


def any_case(n, k, seed, any_nodes, fixed=None, perturbations=None):
    """A network of test_gpu_wide_exact.network with the listed nodes 'any' and seeded constants elsewhere."""
    preds, masks = network(n, k, seed)
    bits = synth.seeded_bits(n, seed + 3)
    chosen = set(any_nodes)
    return yaml_of(preds, masks, ['any' if i in chosen else str(bits[i]) for i in range(n)], fixed=fixed, perturbations=perturbations)


def spread(n, count, seed):
    """`count` node indices: the last node, the nodes 256 .. 259 where the network has them, seeded others."""
    must = {n - 1} | {i for i in range(256, 260) if i < n}
    rest = random.Random(seed).sample([i for i in range(n) if i not in must], count - len(must))
    return sorted(must | set(rest))


def many_attractors_case():
    """n = 1024, every node 'any', and nodes 1000 .. 1015 keep their own value: samples that differ in one of those 16
    bits end in different attractors, so a few hundred samples give more than 256 records."""
    n = 1024
    preds, masks = network(n, 2, 3)
    for i in range(1000, 1016):
        preds[i], masks[i] = [i], 0b10
    return yaml_of(preds, masks, ['any'] * n)


# name -> input text.  L: columns per workgroup (test_gpu_wide_exact.py has the table); a group is 32 L samples.
CASES = {
    # the <= 256-node family: a per-lane handle lowers these a second time on its first sampled call
    'n20': lambda: any_case(20, 2, 2020, range(0, 20, 2), fixed={3: 'any?', 5: '0?'}),
    'n64': lambda: any_case(64, 2, 11, spread(64, 24, 1), fixed={7: '1'}),
    'example2': lambda: open(EXAMPLE2).read(),
    # L = 16
    'n257': lambda: any_case(257, 2, 8, spread(257, 40, 2), fixed={100: '0'}),
    'n300': lambda: any_case(300, 2, 2, spread(300, 40, 3)),
    # L = 8; more 'any' nodes than a bsx_index holds at n = 577; every node 'any' at n = 1024
    'n577': lambda: any_case(577, 2, 31, spread(577, 300, 4), fixed={5: '1'}),
    'n600_9_inputs': lambda: many_preds_case(6),
    'n1024': lambda: any_case(1024, 2, 3, range(1024)),
    'n1024_many_attractors': many_attractors_case,
    # fixed-node variations of radix 3 and 2 (V = 6 from them), an origin schedule and two perturbation variations
    # (radix 3 at t = 9, radix 2 at t = 3): V = 36, T_p = 9 where the 'any?' perturbation is present, else 7
    'n700_variations': lambda: any_case(700, 2, 8, spread(700, 30, 5), fixed={300: 'any?', 650: '0?'},
                                        perturbations={640: {'1': '2, 6-7', 'any?': '9'}, 40: {'0?': '3'}}),
}
L_OF = {'n20': 64, 'n64': 64, 'example2': 64, 'n257': 16, 'n300': 16, 'n577': 8, 'n600_9_inputs': 8, 'n1024': 8, 'n1024_many_attractors': 8,
        'n700_variations': 8}


@functools.lru_cache(maxsize=None)
def compiled(name):
    """-> (net, space, reference), parsed and lowered once per case (simulate mode admits the variations; the engine's
    attract calls take the lowered space whatever mode it was parsed for, as in test_gpu_wide_exact.py)."""
    net, space = compile_problem(parse_input_text(CASES[name](), 100000, Mode.SIMULATE))
    return net, space, WideRef(net, space)


@functools.lru_cache(maxsize=None)
def records(name, first, count, max_t=None, max_len=None, seed=SEED):
    """Per-sample reference records (found, key, lambda, T_p + mu, t_stop) of samples [first, first + count)."""
    net, space, ref = compiled(name)
    return ref.attract(sample_ref.sample_indices(space, seed, range(first, first + count)), max_t, max_len)[0]


def expected(recs):
    """-> (table, number without an attractor, reference steps) as test_gpu_wide_exact.expected_attract."""
    table, none = aggregate(recs)
    return table, none, sum(r[4] for r in recs)


def assert_not_vacuous(generous, split=None):
    found = [r for r in generous if r[0]]
    assert len({r[1] for r in found}) >= 2, 'fewer than two attractors'
    assert any(r[2] > 1 for r in found), 'no cycle longer than 1'
    assert any(r[3] > 0 for r in found), 'no transient'
    if split is not None:
        assert 0 < sum(1 for r in split if r[0]) < len(split), 'the splitting cap does not split'
