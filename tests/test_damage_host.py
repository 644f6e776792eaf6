"""
The flip selection of bsx_run_damage_sampled without a GPU: boolsi_amd/csrc/bsx_sample.h (damage_draw, damage_choose),
position for position against tests/damage_ref.py.  tests/damage_check.cpp is a stand-alone program that the host C++
compiler builds with no HIP include path, so it compiles exactly the functions the kernel calls, and walks samples the way
the kernel does (groups, columns, interleaved masks); it is built a second time with the address and undefined-behaviour
sanitizers and run as its own process.
"""
import itertools
import os
import shutil
import subprocess

import pytest

import damage_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = {'plain': [], 'sanitized': ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']}

N_FREES = [1, 2, 63, 64, 1023, 1024]
FIRSTS = [0, 33, 63, 1000003]           # aligned, inside a block, a column that straddles two blocks, far out
L = 2
COUNT = 32 * L + 37                     # a whole group, then a ragged one
SEED = 7


@pytest.fixture(scope='module')
def programs(tmp_path_factory):
    """kind -> the stand-alone program, built once per kind in pytest's own temporary directory."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    out = {}
    for kind, flags in FLAGS.items():
        out[kind] = str(tmp_path_factory.mktemp('damage_check') / ('damage_check_' + kind))
        subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror'] + flags +
                              ['-I' + os.path.join(ROOT, 'boolsi_amd', 'csrc'), os.path.join(ROOT, 'tests', 'damage_check.cpp'),
                               '-o', out[kind]])
    return out


def run(exe, *args):
    res = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return [[int(v) for v in line.split()[1:]] for line in res.stdout.splitlines()]


def flips_of(n_free):
    return sorted({1, min(2, n_free), min(64, n_free)})


@pytest.mark.parametrize('kind', list(FLAGS))
@pytest.mark.parametrize('n_free', N_FREES)
def test_positions_match_the_definition(programs, kind, n_free):
    seen = set()
    for first, h in itertools.product(FIRSTS, flips_of(n_free)):
        n_any = {1: 0, 2: 1}.get(n_free, n_free - 1)        # the draw's argument depends on it
        lines = run(programs[kind], SEED, first, COUNT, n_any, n_free, h, L)
        assert [line[0] for line in lines] == list(range(first, first + COUNT))
        for line in lines:
            j, got = line[0], line[1:]
            assert got == damage_ref.positions(SEED, j, n_any, n_free, h)
            assert len(set(got)) == h and all(0 <= p < n_free for p in got)
            seen.update(got)
    # not vacuous: the draws spread over the positions (every one is reached where there are few, most where many)
    assert len(seen) == n_free if n_free <= 64 else len(seen) > n_free // 2


@pytest.mark.parametrize('kind', list(FLAGS))
def test_a_full_draw_is_a_permutation(programs, kind):
    """h = n_free: every position is chosen exactly once, whatever the order."""
    for n_free in (1, 2, 33, 64):
        for line in run(programs[kind], SEED, 1000003, 40, 5, n_free, n_free, L):
            assert sorted(line[1:]) == list(range(n_free))
            assert line[1:] == damage_ref.positions(SEED, line[0], 5, n_free, n_free)
    first_orders = {tuple(line[1:]) for line in run(programs[kind], SEED, 1000003, 40, 5, 33, 33, L)}
    assert len(first_orders) == 40
