"""
The part of bsx_run_influence_sampled that needs no device, without a GPU: boolsi_amd/csrc/bsx_influence.h -- the checks of
the arguments, of the source list and of the sizes (every refusal, in the order of the call; the text names the entry and
the node), the cell count, and the (source, group) layout with the item range of every launch -- against a Python model.
tests/influence_check.cpp is a stand-alone program that the host C++ compiler builds with no HIP include path; it is built
a second time with the address and undefined-behaviour sanitizers and run as its own process.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = {'plain': [], 'sanitized': ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']}
OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_RANGE_TOO_LARGE = 0, -1, -4, -9
MAX_CELLS = 1 << 26


@pytest.fixture(scope='module')
def programs(tmp_path_factory):
    """kind -> the stand-alone program, built once per kind in pytest's own temporary directory."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    out = {}
    for kind, flags in FLAGS.items():
        out[kind] = str(tmp_path_factory.mktemp('influence_check') / ('influence_check_' + kind))
        subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror'] + flags +
                              ['-I' + os.path.join(ROOT, 'boolsi_amd', 'csrc'), '-I' + os.path.join(ROOT, 'include'),
                               os.path.join(ROOT, 'tests', 'influence_check.cpp'), '-o', out[kind]])
    return out


def run(exe, *args):
    res = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return res.stdout.splitlines()


def csv_of(values):
    return ','.join(str(v) for v in values) if values else '-'


# ---- checks -------------------------------------------------------------------------------------------------------------

def model_check(n_nodes, fixed, sources, n_steps, first, n_samples, have_table=True, n_sources=None):
    """-> (status, words the text must hold); sources None = NULL.  The order is that of include/bsx.h."""
    n_sources = len(sources) if n_sources is None else n_sources
    if not have_table:
        return ERR_INVALID, ['influence is null']
    if sources is None:
        return ERR_INVALID, ['sources is null']
    if n_sources == 0:
        return ERR_INVALID, ['n_sources']
    if n_steps == 0:
        return ERR_INVALID, ['n_steps']
    if first + n_samples >= 2 ** 64:
        return ERR_INVALID, ['wraps']
    for s, v in enumerate(sources[:n_sources]):
        where = ['sources[{}]'.format(s), 'node {}'.format(v)]
        if v >= n_nodes:
            return ERR_INVALID, where + ['not a node']
        if v in fixed:
            return ERR_INVALID, where + ['fixed by the origin']
        if v in sources[:s]:
            return ERR_INVALID, where + ['twice']
    if n_samples > 2 ** 31:
        return ERR_RANGE_TOO_LARGE, ['2^31']
    if n_sources * n_samples > 2 ** 40:
        return ERR_RANGE_TOO_LARGE, ['2^40']
    if n_sources * n_steps * n_nodes > MAX_CELLS:
        return ERR_UNSUPPORTED, ['BSX_INFLUENCE_MAX_CELLS']
    return OK, []


def check(exe, n_nodes, fixed, sources, n_steps, first, n_samples, have_table=True, n_sources=None):
    count = (0 if sources is None else len(sources)) if n_sources is None else n_sources
    lines = run(exe, 'check', n_nodes, csv_of(sorted(fixed)), 'null' if sources is None else csv_of(sources), count, n_steps, first,
                n_samples, 1 if have_table else 0)
    assert lines[0].startswith('status ') and lines[1].startswith('msg') and lines[2].startswith('cells ')
    return int(lines[0].split()[1]), lines[1][4:], int(lines[2].split()[1])


CALLS = [
    # accepted: one source, every free node in any order, exactly 2^31 samples, 2^40 trajectories, 2^26 cells
    dict(n_nodes=300, fixed={7}, sources=[0], n_steps=12, first=1000003, n_samples=549),
    dict(n_nodes=300, fixed={7}, sources=[299, 0, 8, 6], n_steps=1, first=2 ** 64 - 10, n_samples=9),
    dict(n_nodes=20, fixed=set(), sources=list(range(19, -1, -1)), n_steps=3, first=0, n_samples=0),
    dict(n_nodes=1024, fixed=set(), sources=[5], n_steps=16, first=0, n_samples=2 ** 31),
    dict(n_nodes=1024, fixed=set(), sources=list(range(512)), n_steps=16, first=0, n_samples=2 ** 31),
    dict(n_nodes=1024, fixed={0}, sources=list(range(1, 17)), n_steps=4096, first=0, n_samples=10),
    # refused, each rule alone
    dict(n_nodes=300, fixed={7}, sources=[0], n_steps=12, first=0, n_samples=10, have_table=False),
    dict(n_nodes=300, fixed={7}, sources=None, n_steps=12, first=0, n_samples=10, n_sources=3),
    dict(n_nodes=300, fixed={7}, sources=[0, 1], n_steps=12, first=0, n_samples=10, n_sources=0),
    dict(n_nodes=300, fixed={7}, sources=[0], n_steps=0, first=0, n_samples=10),
    dict(n_nodes=300, fixed={7}, sources=[0], n_steps=12, first=2 ** 64 - 5, n_samples=10),
    dict(n_nodes=300, fixed={7}, sources=[300], n_steps=12, first=0, n_samples=10),
    dict(n_nodes=300, fixed={7}, sources=[3, 4000000000], n_steps=12, first=0, n_samples=10),
    dict(n_nodes=300, fixed={7, 8}, sources=[3, 9, 8], n_steps=12, first=0, n_samples=10),
    dict(n_nodes=300, fixed={7}, sources=[7], n_steps=12, first=0, n_samples=10),
    dict(n_nodes=300, fixed={7}, sources=[3, 9, 3], n_steps=12, first=0, n_samples=10),
    dict(n_nodes=300, fixed={7}, sources=[3, 3], n_steps=12, first=0, n_samples=10),
    dict(n_nodes=1024, fixed=set(), sources=[5], n_steps=16, first=0, n_samples=2 ** 31 + 1),
    dict(n_nodes=1024, fixed=set(), sources=list(range(513)), n_steps=16, first=0, n_samples=2 ** 31),
    dict(n_nodes=1024, fixed={0}, sources=list(range(1, 17)), n_steps=4097, first=0, n_samples=10),
    dict(n_nodes=20, fixed=set(), sources=[0], n_steps=3355444, first=0, n_samples=10),
    dict(n_nodes=20, fixed=set(), sources=[0], n_steps=2 ** 32 - 1, first=0, n_samples=10),
    # the order: null before counts, counts before the wrap, the wrap before the list, the list before the sizes, the range
    # before the cells
    dict(n_nodes=300, fixed={7}, sources=None, n_steps=0, first=2 ** 64 - 1, n_samples=10, have_table=False, n_sources=0),
    dict(n_nodes=300, fixed={7}, sources=[7], n_steps=0, first=2 ** 64 - 1, n_samples=10, n_sources=0),
    dict(n_nodes=300, fixed={7}, sources=[7], n_steps=0, first=2 ** 64 - 1, n_samples=10),
    dict(n_nodes=300, fixed={7}, sources=[7], n_steps=2 ** 30, first=2 ** 64 - 1, n_samples=10),
    dict(n_nodes=300, fixed={7}, sources=[7], n_steps=2 ** 30, first=0, n_samples=2 ** 40),
    dict(n_nodes=300, fixed={7}, sources=[6], n_steps=2 ** 30, first=0, n_samples=2 ** 40),
]


@pytest.mark.parametrize('kind', list(FLAGS))
def test_checks_match_the_model(programs, kind):
    seen = set()
    for call in CALLS:
        status, words = model_check(**call)
        got, text, cells = check(programs[kind], **call)
        assert got == status, (call, text)
        assert all(w in text for w in words), (call, text)
        assert (text == '') == (status == OK)
        n_sources = call.get('n_sources', 0 if call['sources'] is None else len(call['sources']))
        assert cells == min(n_sources * call['n_steps'] * call['n_nodes'], 2 ** 64 - 1)
        seen.add((status, words[-1] if words else ''))
    # every refusal of the call has been met
    assert seen == {(OK, ''), (ERR_INVALID, 'influence is null'), (ERR_INVALID, 'sources is null'), (ERR_INVALID, 'n_sources'),
                    (ERR_INVALID, 'n_steps'), (ERR_INVALID, 'wraps'), (ERR_INVALID, 'not a node'), (ERR_INVALID, 'fixed by the origin'),
                    (ERR_INVALID, 'twice'), (ERR_RANGE_TOO_LARGE, '2^31'), (ERR_RANGE_TOO_LARGE, '2^40'),
                    (ERR_UNSUPPORTED, 'BSX_INFLUENCE_MAX_CELLS')}


@pytest.mark.parametrize('kind', list(FLAGS))
def test_a_list_longer_than_the_network_is_refused_at_its_first_repeat(programs, kind):
    """n_sources may be anything: n + 1 entries cannot be distinct nodes, and no entry behind the offending one is read."""
    got, text, _ = check(programs[kind], 20, set(), list(range(20)) + [4], 3, 0, 10, n_sources=4000000000)
    assert got == ERR_INVALID and 'sources[20]' in text and 'node 4' in text and 'twice' in text


# ---- layout -------------------------------------------------------------------------------------------------------------

def model_layout(n_samples, n_sources, L, chunk):
    G = 32 * L
    g_per = -(-n_samples // G)
    items = g_per * n_sources
    chunk_items = min(max(1, chunk // G), items)
    lines = ['layout {} {} {} {}'.format(G, g_per, items, chunk_items)]
    for p0 in range(0, items, chunk_items):
        count = min(chunk_items, items - p0)
        lines.append('launch {} {}'.format(p0, count))
        for i in range(count):
            s, g = divmod(p0 + i, g_per)
            lines.append('item {} {} {} {} {}'.format(p0 + i, s, g, g * G, min(G, n_samples - g * G)))
    return lines


@pytest.mark.parametrize('kind', list(FLAGS))
@pytest.mark.parametrize('L', [8, 16, 64])
def test_layout_matches_the_model(programs, kind, L):
    G = 32 * L
    for n_samples in (1, G - 1, G, G + 37):
        for n_sources in (1, 3):
            # one group per launch (the clamp of BSX_WIDE_CHUNK = 1), a chunk of two and a half groups, the default
            for chunk in (1, G, 2 * G + G // 2, 1 << 18):
                got = run(programs[kind], 'layout', n_samples, n_sources, L, chunk)
                assert got == model_layout(n_samples, n_sources, L, chunk), (n_samples, n_sources, chunk)
                # every (source, sample) is covered exactly once
                covered = sorted((int(f[2]), int(f[4]) + k) for f in (line.split() for line in got if line.startswith('item'))
                                 for k in range(int(f[5])))
                assert covered == [(s, j) for s in range(n_sources) for j in range(n_samples)]
    # chunk = 1 group: one launch per (source, group)
    got = run(programs[kind], 'layout', G + 37, 3, L, 1)
    assert sum(1 for line in got if line.startswith('launch')) == 6
