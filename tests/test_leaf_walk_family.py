"""
CPU census of the network family of tests/leaf_walk_family.py, which tests/test_gpu_leaf_walk.py runs on the GPU: the
oracle on 2^20 sampled problems of every member confirms what those tests take for granted.
"""
import random

import numpy as np
import pytest

from boolsi_amd.compile import compile_problem
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text
from leaf_walk_family import FAMILY, family_yaml, necklaces


@pytest.mark.parametrize('R,W,D', FAMILY)
def test_the_family_is_what_it_claims_on_the_cpu(R, W, D):
    """Oracle census of 2^20 sampled problems (1024 runs of 1024): one attractor per necklace of the ring, lengths that
    divide R, keys inside the ring bits, mu <= 2."""
    from oracle.cpu_oracle import Oracle, key_int
    n = R + W + D
    net, space = compile_problem(parse_input_text(family_yaml(R, W, D), np.inf, Mode.ATTRACT))
    orc = Oracle(net, space)
    rng = random.Random(n)
    neck = necklaces(R)
    seen = {}
    for _ in range(1024):
        first = rng.randrange((1 << n) - 1024)
        pp, table, none, steps = orc.attract(first, 1024, cap=256)
        assert none == 0 and int(pp['trajectory_l'].max()) <= 2 and bool(pp['found'].all())
        for a in table:
            seen[key_int(a['key'])] = int(a['length'])
    assert seen == neck and all(R % lam == 0 for lam in neck.values())      # (a run of 1024 covers every ring value)
