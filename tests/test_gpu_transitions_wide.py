"""
bsx_run_attractor_transitions_wide / Engine.attractor_transitions_wide: where every single-node flip of every cycle
state of a listed attractor table ends, for networks of every supported size.  Every comparison is exact equality.

References: tests/trans_wide_ref.py above 256 nodes (pinned to tests/trans_ref.py at n <= 256 by
tests/test_trans_wide_ref.py), tests/trans_ref.py itself at n <= 256.  Each case first asserts from the reference alone
that it is not vacuous; the seeds were chosen on the CPU so that those guards hold.  The cases that need their own
environment (BSX_WIDE=1, a lowered BSX_WIDE_STEP_LIMIT, a lowered BSX_WTRANS_CHUNK) run in a fresh child process: this
file, with the case's name and a scratch directory as its arguments; what the child has to reproduce is computed by
the parent and handed over in a file.

Columns per workgroup (see tests/test_gpu_wide_exact.py): L = 16 at n = 257, L = 8 at n = 577 and 1024, L = 64 for the
networks of 11 and 16 nodes under BSX_WIDE=1; a group is 32 * L flips.
"""
import csv
import ctypes as C
import functools
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == '__main__':
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from boolsi_amd import _lib
from boolsi_amd.attract import merge_tables
from boolsi_amd.engine import Engine, EngineError, Stats, ptr

import trans_ref
import trans_wide_ref
import test_gpu_profile as narrow
import test_gpu_wide_exact as wide
from wide_ref import aggregate

pytestmark = pytest.mark.gpu
INF = float('inf')
OUTSIDE, UNRESOLVED = trans_wide_ref.OUTSIDE, trans_wide_ref.UNRESOLVED
assert (OUTSIDE, UNRESOLVED) == (_lib.TRANS_OUTSIDE, _lib.TRANS_UNRESOLVED) == (trans_ref.OUTSIDE, trans_ref.UNRESOLVED)
EXAMPLE2 = os.path.join(ROOT, 'tests', 'golden', 'examples', 'output3_example2', 'example2.yaml')
MAX_FLIPS = 1 << 14


def tuples(edges):
    assert edges.dtype == _lib.TRANS_EDGE and _lib.TRANS_EDGE.itemsize == 24
    return [(int(e['src']), int(e['dst']), int(e['count']), int(e['sum_mu'])) for e in edges]


def check_call(eng, ref, max_t=INF, want=None, launches=None):
    """one call against the reference: edges, node_exits, closed, the row sums and the statistics -> the reference's result"""
    want = want or ref.transitions(max_t)
    edges_want, exits_want, _ = want
    edges, exits, closed = eng.attractor_transitions_wide(ref.keys, ref.lengths, max_t=max_t, node_exits=True)
    got = tuples(edges)
    assert got == edges_want
    assert exits.dtype == np.uint32 and np.array_equal(exits, exits_want)
    assert closed.tolist() == [1] * len(ref.keys)
    for q, length in enumerate(ref.lengths):
        assert sum(e[2] for e in got if e[0] == q) == length * len(ref.free)
    st = eng.trans_stats
    assert st['problems'] == sum(ref.lengths) * len(ref.free) and st['state_steps'] == sum(e[3] for e in got)
    assert st['executed_steps'] >= sum(ref.lengths) + st['state_steps']
    if launches is not None:
        assert st['kernel_launches'] == launches
    edges2, none, _ = eng.attractor_transitions_wide(ref.keys, ref.lengths, max_t=max_t)
    assert none is None and tuples(edges2) == got
    return want


# ---- networks above 256 nodes (pure functions of their arguments: seeds are chosen without a GPU) -----------------------

def wide_text(n, seed, n_any, fixed, many_preds):
    """K = 2 random network with n_any 'any' nodes; `fixed`: {node: '0' / '1'}; many_preds: node n // 2 gets 9
    predecessors, most of them above index 255"""
    preds, masks = wide.network(n, 2, seed)
    if many_preds:
        rng = random.Random(seed + 4)
        node = n // 2
        preds[node] = sorted(rng.sample(range(256), 2) + rng.sample(range(256, n), 7))
        masks[node] = rng.getrandbits(1 << 9)
    return wide.yaml_of(preds, masks, wide.initial(n, seed, n_any, 3), fixed=fixed)


# name: n, seed, 'any' nodes, fixed nodes, a node with 9 predecessors
WIDE_CASES = {
    'n257': (257, 2, 8, {256: '1', 7: '0'}, False),
    'n577': (577, 16, 8, {300: '0'}, True),
    'n1024': (1024, 3, 8, {1000: '1'}, False),
}


@functools.lru_cache(maxsize=None)
def wide_table(name):
    """-> (net, space, [(key, length, frequency)] in the CLI's order) of the attractors the reference finds from every
    initial state of the case"""
    n, seed, n_any, fixed, many = WIDE_CASES[name]
    net, space, ref = wide.compiled(wide_text(n, seed, n_any, fixed, many))
    recs, _ = ref.attract(range(1 << n_any))
    table, none = aggregate(recs)
    assert none == 0
    rows = sorted(((k, e[0], e[1]) for k, e in table.items()), key=lambda r: (-r[2], r[0]))
    return net, space, rows


def budget_rows(rows, n_free, max_flips=MAX_FLIPS):
    """the longest prefix of the table whose flips stay within the budget"""
    out, total = [], 0
    for key, length, _ in rows:
        if (total + length) * n_free > max_flips:
            break
        out.append((key, length))
        total += length
    return out


@functools.lru_cache(maxsize=None)
def wide_ref_of(name):
    net, space, rows = wide_table(name)
    n_free = net.n_nodes - len(WIDE_CASES[name][3])
    keep = budget_rows(rows, n_free)
    ref = trans_wide_ref.TransWideRef(net, space, [k for k, _ in keep], [l for _, l in keep])
    assert len(ref.free) == n_free
    return ref


@pytest.fixture(scope='module')
def eng():
    with Engine(0) as e:
        yield e


# ---- 2. n = 257, 577, 1024 --------------------------------------------------------------------------------------------

def features(ref, want):
    edges, _, detail = want
    return {'fixed_high': any(i > 255 for i in range(ref.n) if ref.fmask[i]),
            'long_row': any(l > 1 for l in ref.lengths),
            'mu_positive': detail['mu_positive'] > 0,
            'cross': len(trans_ref.cross_edges(edges)) > 0}


def test_wide_cases_cover_what_they_must():
    """guards of the three sizes, from the reference alone"""
    seen = {}
    for name in WIDE_CASES:
        ref = wide_ref_of(name)
        want = ref.transitions()
        assert 0 < sum(ref.lengths) * len(ref.free) <= MAX_FLIPS and len(ref.keys) >= 2
        for k, v in features(ref, want).items():
            seen[k] = seen.get(k, False) or v
        assert want[2]['unresolved'] == 0
    assert all(seen.values()), seen
    net = wide_ref_of('n577').net
    assert max(np.diff(net.pred_offsets)) == 9                          # the KW build of the kernel
    assert wide_ref_of('n257').fmask[256] and wide_ref_of('n1024').fmask[1000]


@pytest.mark.parametrize('name', list(WIDE_CASES))
def test_wide_sizes(eng, name):
    ref = wide_ref_of(name)
    want = ref.transitions()
    assert sum(e[2] for e in want[0]) == sum(ref.lengths) * len(ref.free) > 0
    eng.set_problem(ref.net, ref.space)
    assert eng.wide
    # the rows are what attract_wide finds from the case's initial states (in the CLI's order, cut at the flip budget)
    _, _, rows = wide_table(name)
    r = eng.attract_wide(0, 1 << WIDE_CASES[name][2])
    assert {k: (e[0], e[1]) for k, e in merge_tables([r.table]).items()} == {k: (l, f) for k, l, f in rows}
    # profile, the rows' walks, the build, one launch of flips, the drain
    check_call(eng, ref, want=want, launches=5)


# ---- 3. half a table, and a row listed from a non-minimal state ---------------------------------------------------------

def test_half_table_and_a_moved_row(eng):
    full = wide_ref_of('n257')
    full_edges = full.transitions()[0]
    q = next(q for q, l in enumerate(full.lengths) if l > 1)            # guard: a row with more than one state
    keep = sorted({q} | set(range(len(full.keys) // 2)))
    dropped = [d for d in range(len(full.keys)) if d not in keep]
    lost = sum(e[2] for e in full_edges if e[0] in keep and e[1] in dropped)
    assert lost > 0                                                     # guard: edges into dropped rows
    keys = [full.rows[d][1] if d == q else full.keys[d] for d in keep]  # row q from the second state of its cycle
    assert keys[keep.index(q)] != min(full.rows[q])
    ref = trans_wide_ref.TransWideRef(full.net, full.space, keys, [full.lengths[d] for d in keep])
    want = ref.transitions()
    assert want[2]['outside'] >= lost
    eng.set_problem(ref.net, ref.space)
    check_call(eng, ref, want=want)


# ---- 4. caps ----------------------------------------------------------------------------------------------------------

def test_caps(eng):
    full = wide_ref_of('n257')
    half = trans_wide_ref.TransWideRef(full.net, full.space, full.keys[:len(full.keys) // 2], full.lengths[:len(full.keys) // 2])
    outcomes = [half.flip_outcome(x0) for _, _, _, x0 in half.flips()]
    listed = max(mu + lam for _, mu, lam, _, d in outcomes if d is not None)
    unlisted = max(mu + lam for _, mu, lam, _, d in outcomes if d is None)      # guard: there are flips onto unlisted cycles
    caps = sorted({listed, listed - 1, unlisted, unlisted - 1, 0}, reverse=True)
    wants = {c: half.transitions(c) for c in caps}
    # guards: each pair of caps lies on both sides of mu + lambda' of some flip
    assert wants[listed][2]['unresolved'] != wants[listed - 1][2]['unresolved']
    assert wants[unlisted][2]['unresolved'] != wants[unlisted - 1][2]['unresolved']
    assert wants[unlisted][2]['outside'] > wants[unlisted - 1][2]['outside'] or unlisted == listed
    assert wants[0][0] == [(q, UNRESOLVED, l * len(half.free), 0) for q, l in enumerate(half.lengths)]
    eng.set_problem(half.net, half.space)
    for c in [INF] + caps:
        check_call(eng, half, c, wants.get(c))


# ---- 6. refusals --------------------------------------------------------------------------------------------------------

def raw_call(eng, keys, lengths, max_t=INF, edge_cap=64):
    """the ABI call on sentinel-filled outputs -> (status, everything the call may write)"""
    W, n = eng.net.n_words, len(keys)
    key_words = np.zeros((max(n, 1), W), np.uint64)
    for q, k in enumerate(keys):
        key_words[q] = [(int(k) >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(W)]
    lens = np.array(list(lengths) + [0] * (n == 0), np.uint64)
    edges = np.full(edge_cap, 0x5A, np.uint8).repeat(24).view(_lib.TRANS_EDGE)
    exits = np.full((max(n, 1), eng.net.n_nodes), 0x5A5A5A5A, np.uint32)
    closed = np.full(max(n, 1), 0x5A, np.uint8)
    n_edges = C.c_uint64(0x5A5A)
    st = Stats()
    rc = eng._lib.bsx_run_attractor_transitions_wide(eng._h, ptr(key_words), W, ptr(lens), n, _lib.T_INF if max_t == INF else int(max_t),
                                                     edges.ctypes.data_as(C.c_void_p), edge_cap, C.byref(n_edges), ptr(exits), ptr(closed),
                                                     C.byref(st))
    return rc, (edges.tobytes(), exits.tobytes(), closed.tobytes(), n_edges.value), st.as_dict()


def last_error(eng):
    return eng._lib.bsx_last_error(eng._h).decode()


def untouched(eng, n, edge_cap=64):
    return (bytes([0x5A]) * (24 * edge_cap), bytes([0x5A]) * (4 * max(n, 1) * eng.net.n_nodes), bytes([0x5A]) * max(n, 1), 0x5A5A)


def test_refusals(eng):
    ref = wide_ref_of('n257')
    q = next(q for q, l in enumerate(ref.lengths) if l > 1)             # guard
    o = next(d for d in range(len(ref.keys)) if d != q)
    eng.set_problem(ref.net, ref.space)
    cases = {
        'unclosed': ([ref.keys[o], ref.keys[q]], [ref.lengths[o], ref.lengths[q] - 1], 1),
        'duplicate': ([ref.keys[q], ref.keys[o], ref.keys[q]], [ref.lengths[q], ref.lengths[o], ref.lengths[q]], 2),
        'same cycle, another state': ([ref.keys[q], ref.keys[o], ref.rows[q][1]], [ref.lengths[q], ref.lengths[o], ref.lengths[q]], 2),
        'twice the period': ([ref.keys[o], ref.keys[q]], [ref.lengths[o], 2 * ref.lengths[q]], 1),
    }
    for name, (keys, lengths, row) in cases.items():
        rc, out, _ = raw_call(eng, keys, lengths)
        assert rc == _lib.ERR_INVALID and 'row {} '.format(row) in last_error(eng), (name, rc, last_error(eng))
        assert out == untouched(eng, len(keys)), name
        with pytest.raises(EngineError) as err:
            eng.attractor_transitions_wide(keys, lengths, node_exits=True)
        assert err.value.status == _lib.ERR_INVALID and 'row {} '.format(row) in str(err.value), name
    # more cycle states than the limit: 17 rows of 2^24 - 1 (each below the step limit); refused on the host
    rc, out, _ = raw_call(eng, [ref.keys[0]] * 17, [(1 << 24) - 1] * 17)
    assert 17 * ((1 << 24) - 1) > _lib.TRANS_MAX_STATES
    assert rc == _lib.ERR_UNSUPPORTED and 'BSX_TRANS_MAX_STATES' in last_error(eng) and out == untouched(eng, 17)
    rc, out, _ = raw_call(eng, [ref.keys[0]], [0])
    assert rc == _lib.ERR_INVALID and out == untouched(eng, 1)
    # edge_cap
    edges_want = ref.transitions()[0]
    assert len(edges_want) >= 3
    rc, out, _ = raw_call(eng, ref.keys, ref.lengths, edge_cap=len(edges_want) - 1)
    assert rc == _lib.ERR_TABLE_FULL and out == untouched(eng, len(ref.keys), len(edges_want) - 1)
    got, _, _ = eng.attractor_transitions_wide(ref.keys, ref.lengths, edge_cap=len(edges_want))
    assert tuples(got) == edges_want
    # n == 0
    rc, out, st = raw_call(eng, [], [])
    assert rc == 0 and out == untouched(eng, 0) and st['problems'] == 0 and st['kernel_launches'] == 0
    edges, exits, closed = eng.attractor_transitions_wide([], [], node_exits=True)
    assert len(edges) == 0 and exits.shape == (0, 257) and len(closed) == 0


# ---- 7. handle state ----------------------------------------------------------------------------------------------------

def test_handle_state_is_left_alone(eng):
    ref = wide_ref_of('n257')
    eng.set_problem(ref.net, ref.space)
    count = 1 << WIDE_CASES['n257'][2]
    eng.attract_wide(0, count)
    before = eng.attract_wide(0, count)
    eng.attractor_transitions_wide(ref.keys, ref.lengths, node_exits=True)
    after = eng.attract_wide(0, count)
    assert len(before.table) >= 2 and np.array_equal(before.table, after.table) and before.n_no_attractor == after.n_no_attractor
    assert after.stats['executed_steps'] == before.stats['executed_steps'] and after.stats['state_steps'] == before.stats['state_steps']


# ---- 8. host layer and CLI ------------------------------------------------------------------------------------------------

CLI_CASE = (300, 0, 5, {280: '1'})


@functools.lru_cache(maxsize=None)
def cli_case():
    n, seed, n_any, fixed = CLI_CASE
    text = wide_text(n, seed, n_any, fixed, False)
    net, space, ref = wide.compiled(text)
    recs, _ = ref.attract(range(1 << n_any))
    table, none = aggregate(recs)
    assert none == 0
    rows = sorted(((k, e[0], e[1]) for k, e in table.items()), key=lambda r: (-r[2], r[0]))
    return text, trans_wide_ref.TransWideRef(net, space, [r[0] for r in rows], [r[1] for r in rows])


def test_attractor_analysis_on_a_wide_engine(eng):
    from boolsi_amd.attract import AggregatedAttractor
    from boolsi_amd.attractor_analysis import attractor_transitions
    _, ref = cli_case()
    want = ref.transitions()[0]
    assert len(ref.keys) >= 2 and len(want) > len(ref.keys)             # guard: more than the self-loops
    eng.set_problem(ref.net, ref.space)
    assert eng.wide
    attractors = [AggregatedAttractor(k, l, 1, 0, 0) for k, l in zip(ref.keys, ref.lengths)]
    edges, n_free = attractor_transitions(eng, attractors)
    assert tuples(edges) == want and n_free == 299


def run_cli(args, out_dir):
    res = subprocess.run([sys.executable, '-m', 'boolsi_amd'] + args + ['-o', out_dir], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    return res.stdout


def test_cli_transitions_on_300_nodes(tmp_path):
    text, ref = cli_case()
    want = ref.transitions()[0]
    yaml = str(tmp_path / 'n300.yaml')
    with open(yaml, 'w') as f:
        f.write(text)
    run_cli(['attract', yaml], str(tmp_path / 'plain'))
    out = run_cli(['attract', yaml, '--transitions'], str(tmp_path / 'with'))
    assert 'not available' not in out
    plain = sorted(f for f in os.listdir(tmp_path / 'plain') if f.endswith('.csv'))
    assert 'attractor_summaries.csv' in plain and 'attractors.csv' in plain
    assert sorted(f for f in os.listdir(tmp_path / 'with') if f.endswith('.csv')) == sorted(plain + ['attractor_transitions.csv'])
    for name in plain:
        assert open(tmp_path / 'plain' / name, 'rb').read() == open(tmp_path / 'with' / name, 'rb').read(), name
    summaries = list(csv.reader(open(tmp_path / 'with' / 'attractor_summaries.csv')))[1:]
    ids = [r[0] for r in summaries]
    assert [int(r[1]) for r in summaries] == ref.lengths            # guard: the reference's rows are in the CLI's order
    got = open(tmp_path / 'with' / 'attractor_transitions.csv', newline='').read()
    header = 'attractor_id,destination_id,n_perturbations,share,recovery_time_mean'
    assert got == '\r\n'.join([header] + trans_ref.csv_rows(want, ids, ref.lengths, 299)) + '\r\n'


# ---- 1. and 5.: networks of at most 256 nodes on both families; child processes ------------------------------------------

@functools.lru_cache(maxsize=None)
def narrow_ref(name):
    if name == 'example2':
        _, net, space = narrow.compiled(open(EXAMPLE2).read())
        table = narrow.oracle_table(net, space, 8)
    else:
        n, seed, fixed, many = narrow.WIDTH_CASES[name]
        _, net, space = narrow.compiled(narrow.random_text(n, seed, fixed=fixed, many_preds=many))
        table = narrow.oracle_table(net, space, 1 << 10)
    keys = sorted(table)
    return trans_ref.TransRef(net, space, keys, [table[k] for k in keys])


LFSR11 = narrow.block_network(11, [], list(range(10)), 7)               # the 10-bit LFSR and one constant node


@functools.lru_cache(maxsize=None)
def lfsr11_ref():
    assert narrow.lfsr_cycle_length(10, 7) == 1023
    _, net, space = narrow.compiled(LFSR11)
    return trans_ref.TransRef(net, space, [1, 0], [1023, 1])


@functools.lru_cache(maxsize=None)
def mixed_ref():
    net, space, keys, lengths = narrow.mixed_attractors()
    return trans_ref.TransRef(net, space, keys, lengths)


def plain(want):
    edges, exits, _ = want
    return {'edges': [list(e) for e in edges], 'exits': exits.tolist()}


def child(case, tmp_path, expected, env):
    with open(tmp_path / (case + '.json'), 'w') as f:
        json.dump(expected, f)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), case, str(tmp_path)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, **env))
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    assert res.stdout.strip().endswith(case + ' ok')


def call_plain(e, ref, max_t=INF):
    edges, exits, closed = e.attractor_transitions_wide(ref.keys, ref.lengths, max_t=max_t, node_exits=True)
    assert closed.tolist() == [1] * len(ref.keys)
    return {'edges': [list(t) for t in tuples(edges)], 'exits': exits.tolist()}


@pytest.mark.parametrize('name', ['example2', 'n64_fixed'])
def test_families_agree(eng, tmp_path, name):
    ref = narrow_ref(name)
    want = ref.transitions()
    assert len(trans_ref.cross_edges(want[0])) >= 2                     # guard
    if name == 'n64_fixed':
        assert len(ref.free) == 62 and want[1].any()
    eng.set_problem(ref.net, ref.space)
    assert not eng.wide
    old_edges, old_exits, old_closed = eng.attractor_transitions(ref.keys, ref.lengths, node_exits=True)
    assert tuples(old_edges) == want[0] and np.array_equal(old_exits, want[1])
    # without BSX_WIDE the new call is the old one
    check_call(eng, ref, want=want, launches=4)
    new_edges, new_exits, new_closed = eng.attractor_transitions_wide(ref.keys, ref.lengths, node_exits=True)
    assert np.array_equal(new_edges, old_edges) and np.array_equal(new_exits, old_exits) and np.array_equal(new_closed, old_closed)
    # with it, in a child: the reference's result, which is what this process got from the per-lane kernels
    child('agree_' + name, tmp_path, plain((tuples(old_edges), old_exits, None)), {'BSX_WIDE': '1'})


def child_agree(name, expected):
    ref = narrow_ref(name)
    with Engine(0) as e:
        e.set_problem(ref.net, ref.space)
        assert e.wide
        assert call_plain(e, ref) == expected and expected == plain(ref.transitions())
        check_call(e, ref, launches=5)


def test_divergent_walks_in_a_child(tmp_path):
    ref = lfsr11_ref()
    want = ref.transitions()
    # one group is 2048 flips: 11264 are five and a half; the constant node's flips come back after one step
    assert sum(ref.lengths) * len(ref.free) == 11264 and 11264 % 2048 != 0 and want[2]['max_mu'] == 1
    assert want[0] == [(0, 0, 1023 * 11 - 10, 1023), (0, 1, 10, 0), (1, 0, 10, 0), (1, 1, 1, 1)]
    capped = ref.transitions(1023)
    assert 0 < capped[2]['unresolved'] < 11264                           # guard: mu = 1 flips of the cycle need 1024
    mixed = mixed_ref()
    want_mixed = mixed.transitions()
    # 2^20 flips are 512 groups, more than twice the workgroups a launch gets (one per compute unit at this LDS size)
    assert sum(mixed.lengths) * 16 == 1 << 20 and len(want_mixed[0]) == 960
    expected = {'lfsr': plain(want), 'lfsr_capped': plain(capped), 'mixed': plain(want_mixed)}
    child('divergent', tmp_path, expected, {'BSX_WIDE': '1'})


def child_divergent(expected):
    ref, mixed = lfsr11_ref(), mixed_ref()
    with Engine(0) as e:
        e.set_problem(ref.net, ref.space)
        assert e.wide
        assert call_plain(e, ref) == expected['lfsr']
        assert e.trans_stats['kernel_launches'] == 5
        assert call_plain(e, ref, 1023) == expected['lfsr_capped']
        # the same table through several launches of flips: 11264 = 3 * 3000 + 2264, chunks that are no whole groups
        os.environ['BSX_WTRANS_CHUNK'] = '3000'
        assert call_plain(e, ref) == expected['lfsr']
        assert e.trans_stats['kernel_launches'] == 8
        del os.environ['BSX_WTRANS_CHUNK']
        e.set_problem(mixed.net, mixed.space)
        assert call_plain(e, mixed) == expected['mixed']
        os.environ['BSX_WTRANS_CHUNK'] = str(300000)
        assert call_plain(e, mixed) == expected['mixed']
        assert e.trans_stats['kernel_launches'] == 4 + 4


def wide_launches(n, flips, flip_chunk=1 << 22):
    """kernel_launches on the wide family (include/bsx.h): one profile launch per BSX_PROFILE_CHUNK_WIDE rows, the rows'
    walks in launches of 2^18, the build, one launch per flip_chunk flips (2^22, or BSX_WTRANS_CHUNK), the drain"""
    return -(-n // (1 << 18)) + -(-n // (1 << 18)) + 1 + -(-flips // flip_chunk) + 1


def test_three_launches_of_flips_in_a_child(tmp_path):
    ref = wide_ref_of('n257')
    flips = sum(ref.lengths) * len(ref.free)
    chunk = -(-flips // 3)
    assert -(-flips // chunk) == 3 and chunk % (32 * 16)                        # guard: three launches, none of whole groups
    assert wide_launches(len(ref.keys), flips) == 5 and wide_launches(len(ref.keys), flips, chunk) == 7
    n, seed, n_any, fixed, many = WIDE_CASES['n257']
    handed = dict(plain(ref.transitions()), text=wide_text(n, seed, n_any, fixed, many), keys=[str(k) for k in ref.keys],
                  lengths=ref.lengths, launches=7)
    child('chunked', tmp_path, handed, {'BSX_WTRANS_CHUNK': str(chunk)})


def child_chunked(handed):
    net, space, _ = wide.compiled(handed['text'])
    with Engine(0) as e:
        e.set_problem(net, space)
        assert e.wide
        edges, exits, closed = e.attractor_transitions_wide([int(k) for k in handed['keys']], handed['lengths'], node_exits=True)
        assert closed.tolist() == [1] * len(handed['keys'])
        assert [list(t) for t in tuples(edges)] == handed['edges'] and exits.tolist() == handed['exits']
        assert e.trans_stats['kernel_launches'] == handed['launches']


def test_step_limit_in_a_child(tmp_path):
    child('step_limit', tmp_path, {}, {'BSX_WIDE': '1', 'BSX_WIDE_STEP_LIMIT': '512'})


def child_step_limit(expected):
    _, net, space = narrow.compiled(narrow.lfsr_text(10, 7))
    with Engine(0) as e:
        e.set_problem(net, space)
        assert e.wide
        edges, _, _ = e.attractor_transitions_wide([0], [1], max_t=100)     # a cap below a quarter of the limit: decided
        assert tuples(edges) == [(0, UNRESOLVED, 10, 0)]
        try:
            e.attractor_transitions_wide([0], [1])
        except EngineError as err:
            assert err.status == _lib.ERR_STEP_LIMIT, err
        else:
            raise AssertionError('no error')


if __name__ == '__main__':
    case, directory = sys.argv[1], sys.argv[2]
    with open(os.path.join(directory, case + '.json')) as f:
        handed = json.load(f)
    if case.startswith('agree_'):
        child_agree(case[len('agree_'):], handed)
    else:
        {'divergent': child_divergent, 'step_limit': child_step_limit, 'chunked': child_chunked}[case](handed)
    print(case + ' ok')
