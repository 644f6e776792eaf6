"""
boolsi_amd/csrc/bsx_table_lower.cpp without a GPU: the host arithmetic of the calls that take a caller's attractor table
(bsx_run_attractor_profile, bsx_run_node_correlations, bsx_run_attractor_transitions and its _wide twin) -- the checks
of the table, the limits and table sizes of the transition calls, the chunks behind kernel_launches, the device flags
-> status mapping, the finish of the edge list.  A slip in any of them is an out-of-bounds write on the device.

tests/table_lower_check.cpp is a stand-alone program that the host C++ compiler builds together with the unit, with no
HIP include path and -Wall -Wextra -Werror: that it builds this way is the proof that the unit does not depend on HIP.
It is built a second time with the address and undefined-behaviour sanitizers; each build runs as its own process.

The model below is written from the comments of include/bsx.h, not from the unit:
  table      key_stride >= W; at most 2^32 rows; 1 <= length < the family's step limit (2^30; wide: min(2^30,
             BSX_WIDE_STEP_LIMIT), 2^24 by default), a length of 0 reported before a length too long; no key bit at or
             above n_nodes in the W words read; with `states` the ranges [offset, offset + length * W) disjoint, offsets up
             to 2^56, the end of the last one the size of `states`
  sizes      flips = sum of the lengths * free nodes; hash table a power of two >= twice its entries (per lane: the cycle
             states, wide: the rows), at least 2; most edges n (n + 2); edge records min(edge_cap, flips, most edges);
             edge table a power of two >= 2 * that + 2
  launches   one profile launch per BSX_PROFILE_CHUNK (2^22) / BSX_PROFILE_CHUNK_WIDE (2^18) rows; wide: one launch per
             2^18 rows' walks; the build; one launch per 2^28 flips (wide: 2^22, or BSX_WTRANS_CHUNK up to 2^28); the drain
"""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
NO_ROW = 0xFFFFFFFF
OUTSIDE, UNRESOLVED = 0xFFFFFFFE, 0xFFFFFFFF                # BSX_TRANS_OUTSIDE / BSX_TRANS_UNRESOLVED
INVALID, HIP, UNSUPPORTED, TABLE_FULL, STEP_LIMIT = -1, -3, -4, -5, -6
LANES, WIDE = 0, 1
STEP_LIMIT_LANES, STEP_LIMIT_WIDE = 1 << 30, 1 << 24
PROFILE_CHUNK = {LANES: 1 << 22, WIDE: 1 << 18}
ROW_CHUNK, FLIP_CHUNK = 1 << 18, {LANES: 1 << 28, WIDE: 1 << 22}
MAX_STATES = 1 << 28

FLAGS = {'plain': [], 'sanitized': ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']}


def test_status_codes_are_the_header_s():
    text = open(os.path.join(ROOT, 'include', 'bsx.h')).read()
    for name, value in (('BSX_ERR_INVALID', INVALID), ('BSX_ERR_HIP', HIP), ('BSX_ERR_TABLE_FULL', TABLE_FULL),
                        ('BSX_ERR_UNSUPPORTED', UNSUPPORTED), ('BSX_ERR_STEP_LIMIT', STEP_LIMIT)):
        assert '{} = {}'.format(name, value) in ' '.join(text.split()), name


@pytest.fixture(scope='module', params=list(FLAGS))
def check(request, tmp_path_factory):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('table_lower_' + request.param) / 'table_lower_check')
    csrc = os.path.join(ROOT, 'boolsi_amd', 'csrc')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror'] + FLAGS[request.param] +
                          ['-I' + os.path.join(ROOT, 'include'), '-I' + csrc, os.path.join(ROOT, 'tests', 'table_lower_check.cpp'),
                           os.path.join(csrc, 'bsx_table_lower.cpp'), '-o', exe])
    return exe


def ask(exe, lines):
    res = subprocess.run([exe], input='\n'.join(lines) + '\n', capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return [l.split() for l in res.stdout.splitlines()]


def hx(v):
    return format(v, 'x')


def lst(name, values):
    values = list(values)
    return '{} {} {}'.format(name, hx(len(values)), ' '.join(hx(v) for v in values))


def ints(line, name):
    assert line[0] == name, line[:3]
    return [int(v, 16) for v in line[1:]]


def answer(line, name):
    """-> (status, message) of a command that answers with a status"""
    assert line[0] == name
    return int(line[1]), ' '.join(line[2:])


# ----------------------------------------------------------------------------- the table check

class Table:
    """keys as ints of `stride` words, lengths, optional state offsets; what the call is told about the network"""

    def __init__(self, n_nodes, keys, lengths, stride=None, offsets=None, want_states=None, limit=STEP_LIMIT_LANES, null_keys=False):
        self.n_nodes, self.W = n_nodes, (n_nodes + 63) // 64
        self.keys, self.lengths, self.offsets = list(keys), list(lengths), offsets
        self.stride = self.W if stride is None else stride
        self.want_states = (offsets is not None) if want_states is None else want_states
        self.limit, self.null_keys = limit, null_keys

    def commands(self):
        words = [(k >> (64 * w)) & M64 for k in self.keys for w in range(self.stride)]
        return [lst('keys', words), lst('lens', self.lengths), lst('offs', self.offsets or []),
                'check {} {} {} {} {} {} {} {}'.format(hx(self.stride), hx(len(self.lengths)), int(self.null_keys), int(self.want_states),
                                                       int(self.offsets is None), hx(self.W), hx(self.n_nodes), hx(self.limit))]

    def model(self):
        """-> (status, message) or (0, sum_len, state_words)"""
        n, W = len(self.lengths), self.W
        if self.null_keys:
            return INVALID, 'keys or lengths is null'
        if self.want_states and self.offsets is None:
            return INVALID, 'states without state_offsets'
        if self.stride < W:
            return INVALID, 'key_stride is below the words per state'
        if n > 1 << 32:
            return INVALID, 'at most 2^32 attractors per call'
        if 0 in self.lengths:
            return INVALID, 'an attractor of length 0'
        if any(l >= self.limit for l in self.lengths):
            return STEP_LIMIT, 'a walk would exceed the internal step limit'
        if any((k & ((1 << (64 * W)) - 1)) >> self.n_nodes for k in self.keys):
            return INVALID, 'a key has bits at or above n_nodes'
        end = 0
        if self.want_states:
            ranges = sorted((o, o + l * W) for o, l in zip(self.offsets, self.lengths))
            for (_, e0), (o1, _) in zip(ranges, ranges[1:]):
                if o1 < e0:
                    return INVALID, 'state ranges overlap'
            if any(o > 1 << 56 for o, _ in ranges):
                return INVALID, 'state offset out of range'
            end = ranges[-1][1]
        return 0, sum(self.lengths), end


def checked(exe, table):
    line = ask(exe, table.commands())[-1]
    assert line[0] == 'check'
    if line[1] != '0':
        return answer(line, 'check')
    return tuple(ints(line, 'check'))


def test_an_accepted_table_and_a_refusal_for_each_message(check):
    rng = random.Random(1)
    n_nodes = 70
    keys = [rng.getrandbits(n_nodes) for _ in range(5)]
    lengths = [3, 1, 7, 2, 1]
    good = Table(n_nodes, keys, lengths, stride=3, offsets=[20, 0, 40, 26, 2])      # shuffled, touching: 0+2, 2.., 20+6=26, 26+4
    assert good.model() == (0, 14, 40 + 7 * 2)
    assert checked(check, good) == good.model()
    refused = {
        'keys or lengths is null': Table(n_nodes, keys, lengths, null_keys=True),
        'states without state_offsets': Table(n_nodes, keys, lengths, want_states=True),
        'key_stride is below the words per state': Table(n_nodes, [k & M64 for k in keys], lengths, stride=1),
        'an attractor of length 0': Table(n_nodes, keys, [3, 1, 0, 2, 1]),
        'a walk would exceed the internal step limit': Table(n_nodes, keys, [3, 1, 1 << 30, 2, 1]),
        'a key has bits at or above n_nodes': Table(n_nodes, keys[:4] + [keys[4] | 1 << 70], lengths),
        'state ranges overlap': Table(n_nodes, keys, lengths, offsets=[20, 0, 40, 25, 2]),
        'state offset out of range': Table(n_nodes, keys, lengths, offsets=[20, 0, (1 << 56) + 1, 26, 2]),
    }
    statuses = set()
    for message, table in refused.items():
        want = table.model()
        assert want[1] == message
        assert checked(check, table) == want, message
        statuses.add(want[0])
    assert statuses == {INVALID, STEP_LIMIT}
    # a stride of W - 1 words at W = 4
    keys = [rng.getrandbits(250) for _ in range(2)]
    assert checked(check, Table(250, keys, [1, 1], stride=4))[0] == 0
    assert checked(check, Table(250, [k & ((1 << 192) - 1) for k in keys], [1, 1], stride=3)) == (INVALID, 'key_stride is below the words per state')
    # without `states` the offsets are not looked at and state_words is 0
    assert checked(check, Table(n_nodes, [1, 2], [5, 6], stride=2)) == (0, 11, 0)


def test_length_0_is_found_before_a_length_too_long(check):
    for lengths in ([1 << 30, 5, 0], [0, 1 << 30], [5, (1 << 30) + 7, 0, 1 << 31]):
        t = Table(10, [1] * len(lengths), lengths)
        assert t.model() == (INVALID, 'an attractor of length 0') == checked(check, t)
    assert checked(check, Table(10, [1, 1], [M64, 1]))[0] == STEP_LIMIT         # (and no sum wraps on the way)


def test_step_limits_of_both_families(check):
    out = ask(check, ['limit 0 {}'.format(hx(STEP_LIMIT_WIDE)), 'limit 1 {}'.format(hx(STEP_LIMIT_WIDE)), 'limit 1 200', 'limit 0 200'])
    limits = [ints(l, 'limit')[0] for l in out]
    assert limits == [STEP_LIMIT_LANES, STEP_LIMIT_WIDE, 0x200, STEP_LIMIT_LANES]      # the knob is the wide family's alone
    for limit in set(limits):
        ok, bad = Table(300, [1, 2], [1, limit - 1], limit=limit), Table(300, [1, 2], [limit, 1], limit=limit)
        assert checked(check, ok) == (0, limit, 0) == ok.model()
        assert checked(check, bad) == (STEP_LIMIT, 'a walk would exceed the internal step limit') == bad.model()


@pytest.mark.parametrize('n_nodes', [63, 64, 65, 257, 1024])
def test_key_bits_at_or_above_n_nodes(check, n_nodes):
    W = (n_nodes + 63) // 64
    rng = random.Random(n_nodes)
    clean = [rng.getrandbits(n_nodes) | 1 << (n_nodes - 1) for _ in range(3)]
    for stride in (W, W + 2):
        t = Table(n_nodes, clean, [1, 2, 3], stride=stride)
        assert checked(check, t) == (0, 6, 0) == t.model()
        for bit in (n_nodes, 64 * W - 1):
            for q in range(3):
                t = Table(n_nodes, [k | (1 << bit if i == q else 0) for i, k in enumerate(clean)], [1, 2, 3], stride=stride)
                want = t.model()
                # a bit in a word past W (only with a longer stride) is not the call's to judge; bit 64 W - 1 is a node when n_nodes == 64 W
                assert (want[0] == 0) == (bit >= 64 * W or bit < n_nodes), (n_nodes, stride, bit)
                assert checked(check, t) == want, (n_nodes, stride, bit, q)


def test_state_ranges_in_shuffled_order(check):
    rng = random.Random(5)
    W, lengths = 5, [4, 1, 9, 2, 2, 6]
    order = list(range(6))
    for trial in range(6):
        rng.shuffle(order)
        offsets, at = [0] * 6, 3
        for q in order:                                             # touching ranges in a shuffled order, a gap here and there
            offsets[q] = at
            at += lengths[q] * W + (7 if q == 2 else 0)
        t = Table(300, [1] * 6, lengths, offsets=offsets)
        assert t.model() == (0, 24, at - (7 if order[-1] == 2 else 0))
        assert checked(check, t) == t.model()
        for q in order[1:]:                                         # one word back: it overlaps its predecessor
            if order[order.index(q) - 1] == 2:
                continue                                            # (the gap absorbs the word)
            moved = list(offsets)
            moved[q] -= 1
            t = Table(300, [1] * 6, lengths, offsets=moved)
            assert checked(check, t) == (INVALID, 'state ranges overlap') == t.model()
    # equal offsets overlap; the bound of the offsets is 2^56 inclusive
    assert checked(check, Table(300, [1, 1], [1, 1], offsets=[8, 8])) == (INVALID, 'state ranges overlap')
    t = Table(300, [1, 1], [2, 3], offsets=[1 << 56, 0])
    assert checked(check, t) == (0, 5, (1 << 56) + 2 * W) == t.model()
    t = Table(300, [1, 1], [2, 3], offsets=[(1 << 56) + 1, 0])
    assert checked(check, t) == (INVALID, 'state offset out of range') == t.model()


# ----------------------------------------------------------------------------- limits, sizes and plan of the transition calls

def test_transition_limits(check):
    cases = [((5, 9, 1, 1), (0, '')),
             ((5, 9, 0, 1), (INVALID, 'edges or n_edges is null')),
             ((5, 9, 1, 0), (INVALID, 'edges or n_edges is null')),
             (((1 << 32) - 3, 9, 1, 1), (0, '')),
             (((1 << 32) - 2, 9, 1, 1), (INVALID, 'more than 2^32 - 3 attractors')),
             ((5, MAX_STATES, 1, 1), (0, '')),
             ((5, MAX_STATES + 1, 1, 1), (UNSUPPORTED, 'more than 2^28 cycle states (BSX_TRANS_MAX_STATES)')),
             (((1 << 32) - 2, MAX_STATES + 1, 0, 1), (INVALID, 'edges or n_edges is null')),
             (((1 << 32) - 2, MAX_STATES + 1, 1, 1), (INVALID, 'more than 2^32 - 3 attractors'))]
    out = ask(check, ['limits ' + ' '.join(hx(v) for v in args) for args, _ in cases])
    assert [answer(l, 'limits') for l in out] == [want for _, want in cases]


def pow2_at_least(v):
    p = 2
    while p < v:
        p *= 2
    return p


def sizes_model(family, n, sum_len, n_free, edge_cap):
    flips = sum_len * n_free
    slots = pow2_at_least(2 * (n if family == WIDE else sum_len))
    most = n * (n + 2) if n < 1 << 31 else M64
    out_cap = min(edge_cap, flips, most)
    return [flips, slots.bit_length() - 1, slots, most, out_cap, pow2_at_least(2 * out_cap + 2)]


def assert_sizes_sound(family, n, sum_len, got):
    flips, slot_bits, n_slots, most, out_cap, edge_slots = got
    entries = n if family == WIDE else sum_len
    assert n_slots == 1 << slot_bits and n_slots >= 2 and 2 * entries <= n_slots        # a power of two, load <= 1/2
    assert n_slots == 2 or n_slots // 2 < 2 * entries                                   # ... and the least one
    assert edge_slots & (edge_slots - 1) == 0 and edge_slots >= 2
    assert edge_slots >= 2 * (out_cap + 1) and edge_slots // 2 < 2 * (out_cap + 1)      # one edge too many still finds a slot


@pytest.mark.parametrize('family', [LANES, WIDE])
def test_plans(check, family):
    n_nodes = 300 if family == WIDE else 70
    w64, words = (n_nodes + 63) // 64, (n_nodes + 31) // 32
    every = (1 << n_nodes) - 1
    rng = random.Random(11 + family)
    cmds, wants = [], []
    for n in (1, 2, 3, 1000):
        lengths = [rng.choice((1, 1, 2, 5, 17)) for _ in range(n)]
        sum_len = sum(lengths)
        for fixed in (every, every & ~(1 << 65), 0, rng.getrandbits(n_nodes)):
            free = [i for i in range(n_nodes) if not (fixed >> i) & 1]
            exact = min(sum_len * len(free), n * (n + 2))
            for edge_cap in (0, 1, exact, M64):
                cmds += [lst('lens', lengths), lst('fix', [(fixed >> (32 * w)) & 0xFFFFFFFF for w in range(words)]),
                         'plan {} {} {} {}'.format(family, hx(w64), hx(n_nodes), hx(edge_cap))]
                first = [sum(lengths[:q]) for q in range(n)] if n < 10 else None
                wants.append((n, sum_len, free, first, lengths, sizes_model(family, n, sum_len, len(free), edge_cap)))
    out = ask(check, cmds)
    assert len(out) == 4 * len(wants)
    seen_free = set()
    for at, (n, sum_len, free, first, lengths, sizes) in enumerate(wants):
        head, got_free, got_first, got_offsets = out[4 * at:4 * at + 4]
        got = ints(head, 'plan')
        assert got[0] == sum_len and got[1:] == sizes, (n, sizes)
        assert_sizes_sound(family, n, sum_len, got[1:])
        assert ints(got_free, 'free') == free and got[1] == sum_len * len(free)
        seen_free.add(len(free))
        row_first = ints(got_first, 'first')
        assert len(row_first) == n and row_first[0] == 0
        assert [b - a for a, b in zip(row_first, row_first[1:] + [sum_len])] == lengths
        assert first is None or row_first == first
        assert ints(got_offsets, 'offsets') == [f * w64 for f in row_first]
    assert {0, 1, n_nodes} <= seen_free                                         # all fixed (no flips), one free node, all free


def test_sizes_from_the_counts_alone(check):
    cases = [(f, n, s, nf, cap) for f in (LANES, WIDE) for n, s in ((1, 1), (1, 3), (2, 2), (3, 4), (5, 1 << 20), ((1 << 31) - 1, MAX_STATES),
                                                                    (1 << 31, MAX_STATES), ((1 << 32) - 3, MAX_STATES))
             for nf in (0, 1, 1024) for cap in (0, 1, 7, 8, M64)]
    out = ask(check, ['sizes ' + ' '.join(hx(v) for v in c) for c in cases])
    for c, line in zip(cases, out):
        got = ints(line, 'sizes')
        assert got == sizes_model(*c), c
        assert_sizes_sound(c[0], c[1], c[2], got)
    # n (n + 2) fits 64 bits up to n = 2^31 - 1 and saturates from 2^31 on
    most = {c[1]: ints(l, 'sizes')[3] for c, l in zip(cases, out)}
    assert most[(1 << 31) - 1] == ((1 << 31) - 1) * ((1 << 31) + 1) < M64 and most[1 << 31] == M64 == most[(1 << 32) - 3]


# ----------------------------------------------------------------------------- chunks and launch counts

def chunk_pairs(count, chunk):
    return [(at, min(chunk, count - at)) for at in range(0, count, chunk)]


def test_chunks_tile_the_range(check):
    shapes = [(count, chunk) for chunk in (1, 2, 5, 1 << 18, 1 << 28) for count in (0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 5)]
    shapes = [s for s in shapes if s[0] // s[1] < 100]
    out = ask(check, ['chunks {} {}'.format(hx(a), hx(b)) for a, b in shapes])
    for (count, chunk), line in zip(shapes, out):
        got = ints(line, 'chunks')
        pairs = list(zip(got[1::2], got[2::2]))
        assert got[0] == len(pairs) == -(-count // chunk) and pairs == chunk_pairs(count, chunk), (count, chunk)
        assert sum(c for _, c in pairs) == count and all(0 < c <= chunk for _, c in pairs)
        assert [f for f, _ in pairs] == [sum(c for _, c in pairs[:i]) for i in range(len(pairs))]     # each begins where the last ended


def launches_model(family, n, flips, knob):
    flip_chunk = FLIP_CHUNK[family] if family == LANES or not knob else min(knob, 1 << 28)
    profile = -(-n // PROFILE_CHUNK[family])
    rows = -(-n // ROW_CHUNK) if family == WIDE else 0
    return [profile, profile + rows + 1 + -(-flips // flip_chunk) + 1, flip_chunk]


def test_launch_counts(check):
    around = lambda c: (1, c - 1, c, c + 1, 3 * c + 5)
    cases = []
    for family in (LANES, WIDE):
        for n in around(PROFILE_CHUNK[family]):
            cases += [(family, n, flips, 0) for flips in (0,) + around(FLIP_CHUNK[family])]
        cases += [(family, 3, flips, knob) for knob in (1, 3000, 1 << 28, 1 << 29) for flips in (0, 1, 11264, (1 << 29) + 1) if flips // knob < 1 << 20]
    out = ask(check, ['launches ' + ' '.join(hx(v) for v in c) for c in cases])
    for c, line in zip(cases, out):
        assert ints(line, 'launches') == launches_model(*c), c
    # the smallest calls: profile, build, one launch of flips, drain (and the rows' walks on the wide family); no flips, no walk
    assert launches_model(LANES, 3, 50, 0)[1] == 4 and launches_model(WIDE, 3, 50, 0)[1] == 5
    assert launches_model(LANES, 3, 0, 0)[1] == 3 and launches_model(WIDE, 3, 11264, 3000)[1] == 8
    assert launches_model(LANES, 3, 11264, 3000)[1] == 4                       # the knob is the wide family's alone


# ----------------------------------------------------------------------------- the status mapping

def status_model(family, open_row, dup_row, probe, step, overflow, undecided, n_edges, edge_cap):
    wide = family == WIDE
    if open_row != NO_ROW:
        return INVALID, 'row {} is not closed: its key does not return after its length'.format(open_row)
    if dup_row != NO_ROW:
        how = 'lies on the cycle of another row or repeats its own' if wide else 'shares a state with another row or repeats one of its own'
        return INVALID, 'row {} {} (a duplicate row, or a length that is a multiple of the period)'.format(dup_row, how)
    if probe:
        return HIP, 'the row-key table overflowed' if wide else 'the cycle-state table overflowed'
    if step or (wide and undecided):
        return STEP_LIMIT, 'a walk ran into the internal step limit'
    if overflow or n_edges > edge_cap:
        return TABLE_FULL, 'more distinct edges than edge_cap'
    return 0, ''


def test_status_mapping(check):
    clean = dict(open_row=NO_ROW, dup_row=NO_ROW, probe=0, step=0, overflow=0, undecided=0, n_edges=5, edge_cap=5)
    raised = dict(open_row=7, dup_row=0, probe=1, step=3, overflow=1, undecided=2, n_edges=6)
    order = ['open_row', 'dup_row', 'probe', 'step', 'overflow']           # the precedence
    cases = []
    for family in (LANES, WIDE):
        cases.append((family, dict(clean)))
        for name in raised:
            cases.append((family, dict(clean, **{name: raised[name]})))
        for i, a in enumerate(order):
            for b in order[i + 1:] + ['undecided', 'n_edges']:
                cases.append((family, dict(clean, **{a: raised[a], b: raised[b]})))
        cases.append((family, dict(clean, undecided=2, overflow=1)))
        cases.append((family, dict(clean, **raised)))
        cases.append((family, dict(clean, n_edges=0, edge_cap=0)))
        cases.append((family, dict(clean, n_edges=1, edge_cap=0)))
        cases.append((family, dict(clean, open_row=0xFFFFFFFE, dup_row=3)))
    fields = ['open_row', 'dup_row', 'probe', 'step', 'overflow', 'undecided', 'n_edges', 'edge_cap']
    out = ask(check, ['status {} {}'.format(f, ' '.join(hx(c[k]) for k in fields)) for f, c in cases])
    for (family, c), line in zip(cases, out):
        assert answer(line, 'status') == status_model(family, **c), (family, c)
    got = {}                                                                    # by what is raised; the first case of a kind
    for (f, c), l in zip(cases, out):
        got.setdefault((f, tuple(sorted(k for k in c if c[k] != clean[k]))), answer(l, 'status'))
    assert got[LANES, ()] == got[WIDE, ()] == (0, '')                           # n_edges == edge_cap is accepted ...
    assert got[LANES, ('n_edges',)][0] == got[WIDE, ('n_edges',)][0] == TABLE_FULL      # ... and one more is refused
    assert got[LANES, ('undecided',)] == (0, '') and got[WIDE, ('undecided',)][0] == STEP_LIMIT
    assert got[LANES, ('overflow', 'undecided')][0] == TABLE_FULL and got[WIDE, ('overflow', 'undecided')][0] == STEP_LIMIT
    for family in (LANES, WIDE):
        assert 'row 7 ' in got[family, ('open_row',)][1] and 'row 0 ' in got[family, ('dup_row',)][1]
        assert 'row 7 ' in got[family, ('dup_row', 'open_row')][1]
        assert got[family, ('dup_row', 'probe')][0] == INVALID and got[family, ('probe', 'step')][0] == HIP
        assert got[family, ('overflow', 'step')][0] == STEP_LIMIT
    assert got[LANES, ('dup_row',)][1] != got[WIDE, ('dup_row',)][1] and got[LANES, ('probe',)][1] != got[WIDE, ('probe',)][1]


# ----------------------------------------------------------------------------- the edge list

def test_edge_list_finish(check):
    rng = random.Random(9)
    pairs = [(s, d) for s in (0, 1, 5, (1 << 32) - 4) for d in (0, 1, 5, (1 << 32) - 4, OUTSIDE, UNRESOLVED)]
    edges = [(s, d, rng.randrange(1, 1 << 40), 0 if d >= OUTSIDE else rng.randrange(1 << 50)) for s, d in pairs]
    edges.append((9, 9, M64, 1 << 63))                                  # (64-bit fields survive the conversion)
    shuffled = list(edges)
    rng.shuffle(shuffled)
    assert shuffled != sorted(shuffled)
    lists = [shuffled, [], [edges[3]]]
    out = ask(check, ['finish {} {}'.format(hx(len(l)), ' '.join(hx(v) for e in l for v in e)) for l in lists])
    for l, line in zip(lists, out):
        got = ints(line, 'finish')
        assert got[0] == sum(e[3] for e in l) and len(got) == 1 + 4 * len(l)
        assert [tuple(got[1 + 4 * i:5 + 4 * i]) for i in range(len(l))] == sorted(l, key=lambda e: (e[0], e[1]))
