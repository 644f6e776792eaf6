"""
TEST INFRASTRUCTURE -- networks, sample ranges and reference results of the damage-spreading tests
(tests/test_damage_ref.py on the CPU, tests/test_gpu_damage.py and tests/test_gpu_damage_cli.py on the GPU).  Everything is
a pure function of its arguments; the reference of a call is damage_ref.distances over the definition and nothing else.

A range is G + 37 samples from 1000003 (G = 32 L, a group): unaligned, with a ragged second group.  Seed, range and T were
chosen on the CPU so that `expect` is not vacuous for every case and h: distances grow beyond h, the sum moves away from
h * count, and at t = T some pairs have merged and some have not.
"""
import functools
import random

from boolsi_amd.compile import compile_problem
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text

import damage_ref
import sampled_cases
from sampled_cases import FIRST, SEED, any_case, spread
from test_gpu_wide_exact import network, yaml_of
from boolsi_amd import synth
from wide_ref import WideRef

T = 12
FLIPS = (1, 3, 16)


def wide_inputs_case():
    """n = 600, k = 2, except node 123 with 12 and node 300 with 9 predecessors (the per-trajectory table path of the
    kernels); 40 'any' nodes, one fixed node, no variations and no schedule."""
    n = 600
    preds, masks = network(n, 2, 6)
    rng = random.Random(10)
    for node, k, low in ((123, 12, 2), (300, 9, 2)):
        preds[node] = sorted(rng.sample(range(256), low) + rng.sample(range(256, n), k - low))
        masks[node] = rng.getrandbits(1 << k)
    bits = synth.seeded_bits(n, 9)
    chosen = set(spread(n, 40, 6))
    return yaml_of(preds, masks, ['any' if i in chosen else str(bits[i]) for i in range(n)], fixed={50: '1'})


CASES = {name: sampled_cases.CASES[name] for name in ('n64', 'n257', 'n300', 'n577', 'n1024', 'n1024_many_attractors')}
CASES['n600_wide_inputs'] = wide_inputs_case
L_OF = dict({name: sampled_cases.L_OF[name] for name in CASES if name in sampled_cases.L_OF}, n600_wide_inputs=8)
# refused: variations or a schedule
REFUSED = ('n700_variations', 'n600_9_inputs')


@functools.lru_cache(maxsize=None)
def compiled(name):
    """-> (net, space, reference)"""
    if name in sampled_cases.CASES:
        return sampled_cases.compiled(name)
    net, space = compile_problem(parse_input_text(CASES[name](), 100000, Mode.SIMULATE))
    return net, space, WideRef(net, space)


def count_of(name):
    return 32 * L_OF[name] + 37


@functools.lru_cache(maxsize=None)
def distances(name, h, first=FIRST, count=None, steps=T, seed=SEED):
    return damage_ref.distances(compiled(name)[2], seed, first, count_of(name) if count is None else count, h, steps)


@functools.lru_cache(maxsize=None)
def expect(name, h):
    """-> (sum_d, sum_d2, n_merged, hist) of samples [FIRST, FIRST + count_of(name)), T steps, from the reference alone."""
    net, space, ref = compiled(name)
    d = distances(name, h)
    count = count_of(name)
    sum_d, sum_d2, merged, hist = damage_ref.sums(d, net.n_nodes)
    assert sum_d[0] == h * count and merged[0] == 0 and hist[0][h] == count
    assert any(s != h * count for s in sum_d), 'the sum never moves'
    assert int(d.max()) > h, 'no pair exceeds distance h'
    if h in FLIPS:          # (h = 64 at n = 1024 is compared only: no pair merges there)
        assert 0 < merged[T] < count, 'at t = T all pairs have merged, or none'
    return sum_d, sum_d2, merged, hist
