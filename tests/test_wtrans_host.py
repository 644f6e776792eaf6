"""
boolsi_amd/csrc/bsx_wtrans.h without a GPU: the hash of a W-word canonical key, the row-key table and the rule that
turns a flip's walk (found, lambda', mu), its lookup and max_t into an edge, as the wide attractor transitions use
them.  tests/wtrans_check.cpp is a stand-alone program that the host C++ compiler builds with no HIP include path, so
it compiles exactly the functions the kernels call; it is built a second time with the address and undefined-behaviour
sanitizers and run as its own process.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_wtrans_check(tmp_path, extra):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'wtrans_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror'] + extra +
                          ['-I' + os.path.join(ROOT, 'boolsi_amd', 'csrc'), os.path.join(ROOT, 'tests', 'wtrans_check.cpp'), '-o', exe])
    return exe


@pytest.mark.parametrize('flags', [[], ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']],
                         ids=['plain', 'sanitized'])
def test_classification_on_rho_graphs(tmp_path, flags):
    exe = build_wtrans_check(tmp_path, flags)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    word, checks = res.stdout.split()
    # 3 widths x 2 key shapes x 25 x 24 shapes x listed / unlisted x 9 caps x 2 kinds of walk
    assert word == 'ok' and int(checks) == 3 * 2 * 25 * 24 * 2 * 9 * 2
