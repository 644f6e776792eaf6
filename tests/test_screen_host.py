"""
The part of bsx_run_screen_sampled that needs no device, without a GPU: boolsi_amd/csrc/bsx_screen.h -- the validation of
a mutant list (every refusal; the text names the mutant and the node) and the (mutant, group) layout with the pair range of
every launch -- against a Python model.  tests/screen_check.cpp is a stand-alone program that the host C++ compiler builds
with no HIP include path; it is built a second time with the address and undefined-behaviour sanitizers and run as its own
process.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = {'plain': [], 'sanitized': ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']}
OK, ERR_INVALID = 0, -1
MAX_NODES, MAX_MUTANTS = 4, 1 << 20


@pytest.fixture(scope='module')
def programs(tmp_path_factory):
    """kind -> the stand-alone program, built once per kind in pytest's own temporary directory."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    out = {}
    for kind, flags in FLAGS.items():
        out[kind] = str(tmp_path_factory.mktemp('screen_check') / ('screen_check_' + kind))
        subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror'] + flags +
                              ['-I' + os.path.join(ROOT, 'boolsi_amd', 'csrc'), '-I' + os.path.join(ROOT, 'include'),
                               os.path.join(ROOT, 'tests', 'screen_check.cpp'), '-o', out[kind]])
    return out


def run(exe, *args):
    res = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return res.stdout.splitlines()


def csv_of(values):
    return ','.join(str(v) for v in values) if values else '-'


# ---- validation -------------------------------------------------------------------------------------------------------

def model_check(n_nodes, fixed, mutants):
    """-> (status, words the text must hold) of a well-formed list of mutants [(node, value), ...]"""
    if not mutants:
        return ERR_INVALID, ['n_mutants']
    for m, mutant in enumerate(mutants):
        if len(mutant) > MAX_NODES:
            return ERR_INVALID, ['mutant {}'.format(m), 'BSX_SCREEN_MAX_NODES']
    for m, mutant in enumerate(mutants):
        for i, (node, value) in enumerate(mutant):
            where = ['mutant {}'.format(m), 'node {}'.format(node)]
            if node >= n_nodes:
                return ERR_INVALID, where + ['not a node']
            if node in fixed:
                return ERR_INVALID, where + ['fixed by the origin']
            if value > 1:
                return ERR_INVALID, where + ['value above 1']
            if node in [v for v, _ in mutant[:i]]:
                return ERR_INVALID, where + ['twice']
    return OK, []


def check(exe, n_nodes, fixed, mutants, offsets=None, nodes=None, n_mutants=None):
    flat = [pair for m in mutants for pair in m]
    if offsets is None:
        offsets = [0]
        for m in mutants:
            offsets.append(offsets[-1] + len(m))
    nodes = csv_of(['{}:{}'.format(v, c) for v, c in flat]) if nodes is None else nodes
    lines = run(exe, 'check', n_nodes, csv_of(sorted(fixed)), offsets if isinstance(offsets, str) else csv_of(offsets), nodes,
                len(mutants) if n_mutants is None else n_mutants)
    assert lines[0].startswith('status ') and lines[1].startswith('msg')
    return int(lines[0].split()[1]), lines[1][4:]


WELL_FORMED = [
    # accepted
    (300, {7}, [()]),
    (300, {7}, [(), ((0, 0),), ((299, 1),), ((1, 1), (2, 0), (3, 1), (4, 0))]),
    (1024, set(), [((1023, 1),), (), ((0, 0), (1023, 0))]),
    # refused: every rule, at the first and at a later mutant, at the first and at a later node
    (300, {7}, [(), ((300, 0),)]),
    (300, {7}, [((4000000000, 1),)]),
    (300, {7}, [(), ((3, 0),), ((5, 1), (7, 1))]),
    (300, {7, 8}, [((8, 0),)]),
    (300, {7}, [(), ((3, 2),)]),
    (300, {7}, [((3, 1), (4, 4000000000))]),
    (300, {7}, [(), ((3, 0), (9, 1), (3, 1))]),
    (300, {7}, [((3, 0), (3, 0))]),
    (300, {7}, [(), ((1, 1), (2, 0), (3, 1), (4, 0), (5, 0))]),
]


@pytest.mark.parametrize('kind', list(FLAGS))
def test_validation_matches_the_model(programs, kind):
    refused = 0
    for n_nodes, fixed, mutants in WELL_FORMED:
        status, words = model_check(n_nodes, fixed, mutants)
        got, text = check(programs[kind], n_nodes, fixed, mutants)
        assert got == status, (mutants, text)
        assert all(w in text for w in words), (mutants, text)
        assert (text == '') == (status == OK)
        refused += status != OK
    assert refused == 9


@pytest.mark.parametrize('kind', list(FLAGS))
def test_malformed_arrays_are_refused(programs, kind):
    exe = programs[kind]
    two = [(), ((3, 0),)]
    # n_mutants = 0 and above BSX_SCREEN_MAX_MUTANTS (checked before an array is read: the offsets given are short)
    for n_mutants in (0, MAX_MUTANTS + 1):
        got, text = check(exe, 300, set(), two, n_mutants=n_mutants)
        assert got == ERR_INVALID and 'mutants' in text
    # null arrays
    got, text = check(exe, 300, set(), two, offsets='null')
    assert got == ERR_INVALID and 'mut_offsets is null' in text
    got, text = check(exe, 300, set(), two, nodes='null')
    assert got == ERR_INVALID and 'mut_nodes is null' in text
    # (a list of wild types alone needs no nodes)
    assert check(exe, 300, set(), [(), ()], nodes='null') == (OK, '')
    # offsets that do not start at 0, or descend
    got, text = check(exe, 300, set(), two, offsets=[1, 1, 2], nodes='3:0,4:0')
    assert got == ERR_INVALID and 'start at 0' in text
    got, text = check(exe, 300, set(), [(), (), ()], offsets=[0, 2, 1, 2], nodes='3:0,4:0')
    assert got == ERR_INVALID and 'do not ascend' in text and 'mutant 1' in text


# ---- layout -------------------------------------------------------------------------------------------------------------

def model_layout(n_samples, n_mutants, L, chunk):
    G = 32 * L
    g_per = -(-n_samples // G)
    pairs = g_per * n_mutants
    chunk_pairs = min(max(1, chunk // G), pairs)
    lines = ['layout {} {} {} {}'.format(G, g_per, pairs, chunk_pairs)]
    for p0 in range(0, pairs, chunk_pairs):
        count = min(chunk_pairs, pairs - p0)
        lines.append('launch {} {}'.format(p0, count))
        for i in range(count):
            m, g = divmod(p0 + i, g_per)
            lines.append('pair {} {} {} {} {}'.format(p0 + i, m, g, min(G, n_samples - g * G), i * G))
    return lines


@pytest.mark.parametrize('kind', list(FLAGS))
@pytest.mark.parametrize('L', [8, 16, 64])
def test_layout_matches_the_model(programs, kind, L):
    G = 32 * L
    for n_samples in (1, G - 1, G, G + 37):
        for n_mutants in (1, 3):
            # one group per launch (the clamp of BSX_WIDE_CHUNK = 1), a chunk of two and a half groups, the default
            for chunk in (1, G, 2 * G + G // 2, 1 << 18):
                got = run(programs[kind], 'layout', n_samples, n_mutants, L, chunk)
                assert got == model_layout(n_samples, n_mutants, L, chunk), (n_samples, n_mutants, chunk)
                # every (mutant, sample) is covered exactly once
                covered = sorted((int(f[2]), int(f[3]) * G + k) for f in (line.split() for line in got if line.startswith('pair'))
                                 for k in range(int(f[4])))
                assert covered == [(m, j) for m in range(n_mutants) for j in range(n_samples)]
    # chunk = 1 group: one launch per (mutant, group)
    got = run(programs[kind], 'layout', G + 37, 3, L, 1)
    assert sum(1 for line in got if line.startswith('launch')) == 6
