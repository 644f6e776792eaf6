"""
The workgroup prologue's staging (`stage_network`, the pool kernel's mirror image and per-parent rule table) at the edges of
its copy loops, every thread copying 16-byte items in rounds of one block.  The cases are chosen by copy size, not by
workload: fewer items than a round has threads, a ragged last round, a whole number of rounds, many rounds; mirrors from 64
slots to more slots than a workgroup has threads.  Every case runs through every build that stages: plain enumeration, the
cube top, the lower levels per child and per parent under a forced depth of 2 and 3 -- each also with BSX_MIRROR_IMAGE=0
(no image: the mirror is regenerated in LDS) and with BSX_CUBE_LOWER=0 (the general cube build on the lower levels).
(Written for the batched staging of DESIGN.md section 5 "The launch floor", which is not in; the cases hold for any copy.)

Expected results: the CPU oracle for the random networks (table, no-attractor count, reference steps), the closed form for
the `family_yaml` networks (one attractor per necklace of the ring, basin = space / 2^R).
"""
import os
import re

import numpy as np
import pytest

from boolsi_amd import synth
from boolsi_amd.attract import merge_tables
from boolsi_amd.compile import compile_problem
from boolsi_amd.constants import Mode
from boolsi_amd.engine import key_to_int
from boolsi_amd.input import parse_input_text
from leaf_walk_family import family_yaml, necklaces

pytestmark = pytest.mark.gpu
CORES = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
KNOBS = ('BSX_CUBES', 'BSX_CUBE_DEPTH', 'BSX_CUBE_LEAF', 'BSX_CUBE_LOWER', 'BSX_MIRROR_IMAGE', 'BSX_CACHE_LDS_KB', 'BSX_LUT_MODE', 'BSX_DEBUG')

BUILDS = [('plain', {'BSX_CUBES': '0'}),
          ('cube top', {}),
          ('per child, depth 2', {'BSX_CUBE_LEAF': '0', 'BSX_CUBE_DEPTH': '2'}),
          ('per child, depth 3', {'BSX_CUBE_LEAF': '0', 'BSX_CUBE_DEPTH': '3'}),
          ('per parent, depth 2', {'BSX_CUBE_DEPTH': '2'}),
          ('per parent, depth 3', {'BSX_CUBE_DEPTH': '3'})]
EXTRAS = [{}, {'BSX_MIRROR_IMAGE': '0'}, {'BSX_CUBE_LOWER': '0'}]


@pytest.fixture()
def knobs():
    yield
    for k in KNOBS:
        os.environ.pop(k, None)


def every_build():
    """Sets the environment of one build after the other: -> (label, the knobs set)."""
    for label, build in BUILDS:
        for extra in EXTRAS:
            env = dict(build, **extra)
            os.environ.update(env)
            try:
                yield '{} {}'.format(label, extra or ''), env
            finally:
                for k in env:
                    os.environ.pop(k, None)


def rows(table):
    return sorted((key_to_int(a['key']), int(a['length']), int(a['count']), int(a['sum_l']),
                   int(a['sum_l2_lo']) + (int(a['sum_l2_hi']) << 64)) for a in table)


# n, K, seed, knobs read by set_problem, the LUT mode that gives (1 bytes, 2 nibbles, 0 not staged), first, count, max_t -- and
# the LUT copy the case exercises (16-byte items; 768 threads in the pool kernel, 256 to 1024 in the others).  Ranges are
# aligned blocks of 2^16 problems, the smallest a cube pass takes (n = 8 has 2^8 problems in all: plain kernels only).
# K = 3 at n = 64 is a chaotic network: a cap keeps the oracle quick.  The byte table of n = 128 takes 128 KiB of LDS, which
# the library grants only next to a small cycle cache (BSX_CACHE_LDS_KB=8); left alone it picks the nibble table.
CASES = [
    ('n8_k1', 8, 1, 81, {}, 1, 0, 1 << 8, 4096),                            # 64 items: less than one round of any block
    ('n24_k2', 24, 2, 242, {}, 1, 5 << 16, 1 << 16, 4096),                  # 384 items
    ('n64_k2', 64, 2, 64, {}, 1, 0x9E3779B97F4A << 16, 1 << 16, 4096),      # 2048 items: ragged last round (the north star)
    ('n64_k3', 64, 3, 643, {}, 1, 0x9E3779B97F4A << 16, 1 << 16, 256),      # 3072 items = 4 x 768, two-plane entries
    ('n128_k2', 128, 2, 129, {'BSX_CACHE_LDS_KB': '8'}, 1, 0x51F15E << 16, 1 << 16, 4096),     # 8192 items: many rounds, four-word build
    ('n128_k2_nibble', 128, 2, 129, {'BSX_LUT_MODE': '2'}, 2, 0x51F15E << 16, 1 << 16, 4096),  # ... as a nibble table: 1024 items
    ('n64_k2_global', 64, 2, 64, {'BSX_LUT_MODE': '0'}, 0, 0x9E3779B97F4A << 16, 1 << 16, 4096),   # table not staged: masks only
]


@pytest.mark.parametrize('name,n,k,seed,setup,lut_mode,first,count,max_t', CASES, ids=[c[0] for c in CASES])
def test_lut_copy_sizes_against_the_oracle(knobs, name, n, k, seed, setup, lut_mode, first, count, max_t):
    from boolsi_amd.engine import Engine
    from oracle.cpu_oracle import Oracle
    net, space = compile_problem(parse_input_text(synth.network_yaml(n, k, seed), max_t, Mode.ATTRACT))
    _, table, none, steps = Oracle(net, space).attract(first, count, max_t, None, per_problem=False, n_threads=CORES)
    want = rows(table)
    os.environ.update(setup)
    with Engine(0) as eng:
        eng.set_problem(net, space)
        for key in setup:
            os.environ.pop(key)
        print(name, eng.network_info())
        assert eng.network_info()['lut_mode'] == lut_mode
        for label, _ in every_build():
            got = eng.attract(first, count, max_t)
            assert rows(got.table) == want, label
            assert got.n_no_attractor == none and got.stats['state_steps'] == steps, label


# R, BSX_CACHE_LDS_KB, slots of the mirror once all 2^R cycle states are cached (a cube pass keeps two entries per state, at
# two to four slots per entry; 1 KiB = 64 slots, 4 KiB = 256 slots of 16 bytes); W = 6 layer-1 and D layer-0 nodes make whole
# spaces of 2^22 to 2^24 problems
MIRRORS = [(4, 1, 64, 12), (6, 4, 256, 12), (6, None, 512, 12), (7, None, 1024, 11)]


@pytest.mark.parametrize('R,lds_kb,slots,D', MIRRORS, ids=['slots{}'.format(m[2]) for m in MIRRORS])
def test_mirror_sizes_in_closed_form(knobs, capfd, R, lds_kb, slots, D):
    """64 slots: less than one round of the image copy; 1024 slots: more slots than a workgroup has threads (several rounds of
    the image copy, two of the per-parent level's compaction)."""
    from boolsi_amd.engine import Engine
    W = 6
    total = 1 << (R + W + D)
    if lds_kb:
        os.environ['BSX_CACHE_LDS_KB'] = str(lds_kb)    # (read by every set_problem: stays for the whole test)
    net, space = compile_problem(parse_input_text(family_yaml(R, W, D), np.inf, Mode.ATTRACT))
    want = {key: [lam, lam << (W + D)] for key, lam in necklaces(R).items()}
    with Engine(0) as eng:
        eng.set_problem(net, space)
        eng.attract2(0, total)                          # (first contact with the attractors: the mirror grows with the cache)
        capfd.readouterr()
        first_outcome, lower = None, {}
        for label, env in every_build():
            os.environ['BSX_DEBUG'] = '1'
            got = eng.attract2(0, total)
            os.environ.pop('BSX_DEBUG')
            seen = re.findall(r'\[bsx\] mirror: (\d+) cycle states cached, (\d+) slots', capfd.readouterr().err)
            # (a plain pass has no representative entries, so half the entries and possibly a smaller mirror)
            assert seen and all(int(c) == 1 << R and (int(m) == slots or (int(m) < slots and 'BSX_CUBES' in env)) for c, m in seen), (label, seen)
            merged = merge_tables([got.table])
            assert {key: v[:2] for key, v in merged.items()} == want, label
            assert got.n_no_attractor == 0, label
            outcome = (merged, got.stats['state_steps'])
            first_outcome = first_outcome or outcome    # (the sums of l and l^2 and the reference steps: all builds alike)
            assert outcome == first_outcome, label
            lower[tuple(sorted(env.items()))] = got.stats['lower_executed_steps']
        # the per-parent level did run where it was asked for: one update per parent against one per child
        # (with the image and the lower-level build, that is: the level is part of that build)
        for depth in '23':
            per_parent = (('BSX_CUBE_DEPTH', depth),)
            per_child = (('BSX_CUBE_DEPTH', depth), ('BSX_CUBE_LEAF', '0'))
            assert lower[per_parent] < lower[per_child], (depth, lower)
