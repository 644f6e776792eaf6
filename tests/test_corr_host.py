"""
Host side of the node correlations, checked without a GPU: the rank arithmetic of boolsi_amd/csrc/bsx_ranks.h (tie-group
bounds -> rank2 -> d2, and the total frequency with its refusals).  tests/corr_check.cpp is a stand-alone program that
the host C++ compiler builds with no HIP include path, so it compiles exactly the functions the kernels call; it is
built a second time with the address and undefined-behaviour sanitizers and run as its own process.
Also here: the size rule of find_node_correlations, which needs no device to be decided.
"""
import os
import shutil
import subprocess

import pytest

from boolsi_amd import attractor_analysis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_corr_check(tmp_path, extra):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'corr_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror'] + extra +
                          ['-I' + os.path.join(ROOT, 'boolsi_amd', 'csrc'), os.path.join(ROOT, 'tests', 'corr_check.cpp'), '-o', exe])
    return exe


@pytest.mark.parametrize('flags', [[], ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']],
                         ids=['plain', 'sanitized'])
def test_ranks_count_like_pairs(tmp_path, flags):
    exe = build_corr_check(tmp_path, flags)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    word, compared = res.stdout.split()
    assert word == 'ok' and int(compared) > 4_000       # (six sizes, four tie patterns, three kinds of weights)


def test_size_rule():
    cells = attractor_analysis.DEVICE_CORRELATION_CELLS
    assert cells >= 1 << 12 and cells & (cells - 1) == 0
    engine = object()
    assert not attractor_analysis.uses_device(cells // 64 - 1, 64, engine)
    assert attractor_analysis.uses_device(cells // 64, 64, engine)
    assert not attractor_analysis.uses_device(1 << 20, 64, None)             # no engine: the host path, whatever the size
    assert attractor_analysis.uses_device(2, 2, engine, device=True) and not attractor_analysis.uses_device(1 << 20, 64, engine, device=False)
