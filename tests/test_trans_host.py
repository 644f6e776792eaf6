"""
Host side of the attractor transitions, checked without a GPU: the walking lane's decision logic of
boolsi_amd/csrc/bsx_walk.h (Brent's detector with power-of-two checkpoints, hits on listed cycles, the mu pass for
unlisted ones, the early stop under a cap and the step limit).  tests/trans_check.cpp is a stand-alone program that the
host C++ compiler builds with no HIP include path, so it compiles exactly the function the kernel calls; it is built a
second time with the address and undefined-behaviour sanitizers and run as its own process.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_trans_check(tmp_path, extra):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'trans_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror'] + extra +
                          ['-I' + os.path.join(ROOT, 'boolsi_amd', 'csrc'), os.path.join(ROOT, 'tests', 'trans_check.cpp'), '-o', exe])
    return exe


@pytest.mark.parametrize('flags', [[], ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']],
                         ids=['plain', 'sanitized'])
def test_walker_on_rho_graphs(tmp_path, flags):
    exe = build_trans_check(tmp_path, flags)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    word, walks = res.stdout.split()
    assert word == 'ok' and int(walks) > 60_000         # (41 x 40 shapes, listed and unlisted, some twenty caps and limits each)
