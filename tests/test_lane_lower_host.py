"""
boolsi_amd/csrc/bsx_lane_lower.cpp without a GPU: what the per-lane family's host side (n <= 256) makes of a network, a
problem space and a call before anything is uploaded or launched -- the gather LUT in its three layouts, the truth-table
masks, the LDS budget that picks the LUT mode, the host part of DevSpace, the dense schedule, the deposit plan, the variant
count, the problem-index arithmetic, a variant's fixed nodes, the counting plan of bsx_run_target_summary and the shapes
of the simulate launches.

tests/lane_lower_check.cpp is a stand-alone program that the host C++ compiler builds together with the unit, with no
HIP include path and -Wall -Wextra -Werror: that it builds this way is the proof that the unit does not depend on HIP.
It is built a second time with the address and undefined-behaviour sanitizers; each build runs as its own process.

The model below is written from the layout comments of bsx_device.h (DevNet, DevSpace, SlicedParams) and bsx.h:
  masks [1 << k_mux][nw]: bit i = TT_i(idx), the table replicated over the slots node i does not use; 0 for a node with
  more than 6 predecessors.  lut [chunk][value][slot j][word w]: the bits i whose j-th predecessor lies in the chunk (8
  state bits, 4 in nibble mode) and is set in `value`; an entry of 6 words is stored in two planes, words 0..3 of every
  entry and then words 4..5, unless the mode is the nibble one.  The LUT is in LDS while masks + LUT + cache mirror + 64
  bytes fit 144 KiB: whole bytes (mode 1), else nibbles for nw >= 4 (mode 2), else it stays in HBM (mode 0).
  Deposit run r: digits [src, src + len) -> bits [shift, shift + len) of word `word`, packed src | word << 8 | shift << 16
  and (1 << len) - 1.

Two cases the layouts rule out are noted where they would stand: a nibble table with k_mux * nw == 6 (nibbles need
nw >= 4) and more than kMaxDepositRuns runs with n_any <= 64 (a run holds at least one node).
"""
import os
import random
import shutil
import subprocess

import pytest

from boolsi_amd import batching
from boolsi_amd.constants import RANGE_CODE, NodeStateRange

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
MAX_W32, MAX_RUNS, MAX_MUX_K = 8, 64, 6                                     # bsx_device.h
CACHE_LDS_BYTES, STEP_LIMIT, BLOCK = 16 * 1024, 1 << 30, 512
CUBE_MIN_BITS, CUBE_MAX_BITS = 16, 63                                       # bsx_cube_plan.h
INVALID, UNSUPPORTED = -1, -4
ANY_Q = 3                                                                   # BSX_RANGE_MAYBE_TRUE_OR_FALSE, radix 3

FLAGS = {'plain': [], 'sanitized': ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']}


@pytest.fixture(scope='module', params=list(FLAGS))
def check(request, tmp_path_factory):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('lane_lower_' + request.param) / 'lane_lower_check')
    csrc = os.path.join(ROOT, 'boolsi_amd', 'csrc')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror'] + FLAGS[request.param] +
                          ['-I' + os.path.join(ROOT, 'include'), '-I' + csrc, os.path.join(ROOT, 'tests', 'lane_lower_check.cpp'),
                           os.path.join(csrc, 'bsx_lane_lower.cpp'), '-o', exe])
    return exe


def ask(exe, lines):
    res = subprocess.run([exe], input='\n'.join(lines) + '\n', capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return [l.split() for l in res.stdout.splitlines()]


def hx(v):
    return format(v, 'x')


def cmd(name, *values):
    return ' '.join([name] + [hx(int(v)) for v in values])


def lst(name, values, per=1):
    values = list(values)
    return '{} {} {}'.format(name, hx(len(values) // per), ' '.join(hx(v) for v in values))


def ints(line, name):
    assert line[0] == name, line[:3]
    return [int(v, 16) for v in line[1:]]


def failure(line, name):
    """-> (status, message) of a refused command"""
    assert line[0] == name
    return int(line[1]), ' '.join(line[2:])


def words(value, n, bits=32):
    """an int as n little-endian words of `bits` bits; it must fit them (linear in its size, unlike shifting word by word)"""
    raw = value.to_bytes(n * bits // 8, 'little')
    return [int.from_bytes(raw[at:at + bits // 8], 'little') for at in range(0, len(raw), bits // 8)]


def round_up(v, m):
    return -(-v // m) * m


# ----------------------------------------------------------------------------- the network

class Net:
    """preds[i] ascending, tables[i] node i's whole truth table as an int"""

    def __init__(self, n, preds, tables):
        self.n, self.preds, self.tables = n, preds, tables
        self.nw = 1 if n <= 32 else 2 if n <= 64 else 4 if n <= 128 else 8
        self.w64 = (n + 63) // 64
        self.mux = [i for i in range(n) if len(preds[i]) <= MAX_MUX_K]
        self.K = max([1] + [len(preds[i]) for i in self.mux])

    def commands(self, cache_kb=0, lut=None):
        tt_words = [max(1, (1 << len(p)) // 64) for p in self.preds]
        po = [sum(len(p) for p in self.preds[:i]) for i in range(self.n + 1)]
        tto = [sum(tt_words[:i]) for i in range(self.n + 1)]
        tt = [w for t, nwords in zip(self.tables, tt_words) for w in words(t, nwords, 64)]
        return [lst('po', po), lst('pi', [p for ps in self.preds for p in ps]), lst('tto', tto), lst('tt', tt),
                cmd('net', self.n, cache_kb, 0 if lut is None else lut + 1)]

    def lds(self, cache_kb=0):
        """-> mask bytes, cache stride, slots, cache bytes (the mirror, its header and the lean kernel's tables)"""
        mask_bytes = round_up((1 << self.K) * self.nw, 4) * 4
        stride = round_up(2 * self.nw + 2, 4) * 4
        budget = cache_kb * 1024 if cache_kb else CACHE_LDS_BYTES
        slots = 1
        while slots * 2 * stride <= budget:
            slots *= 2
        lean = 64 * (8 + 8 + 4 + 4 + 4 * self.nw) + 16 + 8 * (256 + 256)
        return mask_bytes, stride, slots, slots * stride + 32 + lean

    def mode(self, cache_kb=0, forced=None):
        mask_bytes, _, _, cache_bytes = self.lds(cache_kb)
        entry = self.K * self.nw * 4
        room = 144 * 1024 - (mask_bytes + cache_bytes + 64)
        nibbles = self.nw >= 4 and self.nw * 8 * 16 * entry <= room
        mode = 1 if self.nw * 4 * 256 * entry <= room else 2 if nibbles else 0
        if forced == 0 or (forced == 2 and nibbles):
            mode = forced
        return mode

    def model(self, cache_kb=0, forced=None):
        n, nw, K = self.n, self.nw, self.K
        mode = self.mode(cache_kb, forced)
        mask_bytes, stride, slots, cache_bytes = self.lds(cache_kb)
        masks = []
        for idx in range(1 << K):
            row = sum(((self.tables[i] >> (idx % (1 << len(self.preds[i])))) & 1) << i for i in self.mux)
            masks += words(row, nw)
        cb = 4 if mode == 2 else 8
        n_chunks = nw * 32 // cb
        # who[j][p]: the nodes (as a bit set) whose j-th predecessor is node p
        who = [[0] * (nw * 32) for _ in range(K)]
        for i in self.mux:
            for j, p in enumerate(self.preds[i]):
                who[j][p] |= 1 << i
        entries = []
        for chunk in range(n_chunks):
            for value in range(1 << cb):
                entry = []
                for j in range(K):
                    entry += words(sum(who[j][chunk * cb + b] for b in range(cb) if (value >> b) & 1), nw)
                entries.append(entry)
        if K * nw == 6 and mode != 2:
            lut = [w for e in entries for w in e[:4]] + [w for e in entries for w in e[4:]]
        else:
            lut = [w for e in entries for w in e]
        wide = [i for i in range(n) if len(self.preds[i]) > MAX_MUX_K]
        wdesc, wpreds, wtt = [], [], []
        for i in wide:
            k = len(self.preds[i])
            wdesc += [i, k, len(wpreds), len(wtt)]
            wpreds += self.preds[i]
            wtt += words(self.tables[i], (1 << k) // 32)
        shmem = mask_bytes + (len(lut) * 4 if mode else 0) + 64
        return dict(head=[nw, K, n_chunks, len(wide), mode, slots, stride, cache_bytes, shmem, shmem + cache_bytes],
                    masks=masks, lut=lut, wdesc=wdesc, wpreds=wpreds, wtt=wtt,
                    mpo=[sum(len(p) for p in self.preds[:i]) for i in range(n + 1)], mpi=[p for ps in self.preds for p in ps],
                    mtt0=[t & M64 for t in self.tables])


NET_FIELDS = ['net', 'masks', 'lut', 'wdesc', 'wpreds', 'wtt', 'mpo', 'mpi', 'mtt0']


def lowered_net(check, net, cache_kb=0, lut=None):
    out = ask(check, net.commands(cache_kb, lut))
    assert [l[0] for l in out] == NET_FIELDS
    got = {l[0]: ints(l, l[0]) for l in out}
    got['head'] = got.pop('net')
    return got


def network(n, K, seed, extra=()):
    """node i has 1 + i % K predecessors (so most nodes use fewer than K slots), node 0 has K; extra: (node, k) overrides"""
    rng = random.Random(seed)
    counts = [min(n, 1 + i % K) for i in range(n)]
    counts[0] = min(n, K)
    for node, k in extra:
        counts[node] = k
    preds = [sorted(rng.sample(range(n), k)) for k in counts]
    return Net(n, preds, [rng.getrandbits(1 << len(p)) for p in preds])


SIZES = (1, 31, 32, 33, 64, 65, 128, 129, 256)


def test_case_mix():
    modes = {(n, K): network(n, K, 1).mode() for n in SIZES for K in range(1, 7)}
    assert set(modes.values()) == {0, 1, 2}
    assert {network(n, 1, 1).nw for n in SIZES} == {1, 2, 4, 8}
    assert modes[128, 1] == 1 and modes[128, 2] == 2 and modes[256, 3] == 2 and modes[256, 4] == 0
    # the planar layout: k_mux * nw == 6 happens at nw = 1 and nw = 2 only, where the nibble mode does not exist
    assert network(40, 3, 1).mode() == 1 and network(20, 6, 1).mode() == 1
    assert all(nw * K != 6 for nw in (4, 8) for K in range(1, 7))


@pytest.mark.parametrize('n', SIZES)
def test_network_tables_equal_the_model_at_every_width_and_slot_count(check, n):
    for K in range(1, 7):
        if K > n:
            continue
        # 7 and more predecessors: absent from masks and LUT (a table of 2^24 bits is 2^18 words to print: one case carries it)
        extra = [(n // 2, 7), (n - 1, 24 if (n, K) == (65, 2) else 9)] if n >= 31 and K in (2, 5) else []
        net = network(n, K, 100 * n + K, extra)
        assert net.K == K and (not extra or len(net.mux) == n - 2)
        got, want = lowered_net(check, net), net.model()
        for field in want:
            assert got[field] == want[field], (n, K, field)


def test_lut_modes_forced_and_refused(check):
    cases = [(network(40, 3, 1), None, 1), (network(40, 3, 1), 0, 0),       # planar, in LDS and in HBM
             (network(40, 3, 1), 2, 1),                                      # no nibbles below 128 nodes: stays planar bytes
             (network(20, 6, 2), None, 1), (network(20, 6, 2), 0, 0),       # planar at nw = 1
             (network(100, 1, 3), None, 1), (network(100, 1, 3), 2, 2), (network(100, 1, 3), 0, 0),
             (network(100, 3, 4), None, 2), (network(100, 3, 4), 0, 0),
             (network(200, 3, 5), None, 2), (network(200, 4, 6), None, 0),
             (network(200, 4, 6), 2, 0), (network(256, 6, 7), 2, 0)]        # a forced 2 without the room for it
    for net, forced, mode in cases:
        want = net.model(forced=forced)
        assert want['head'][4] == mode
        got = lowered_net(check, net, lut=forced)
        for field in want:
            assert got[field] == want[field], (net.n, net.K, forced, field)
    # the two planes differ from the interleaved layout whenever a word 4 or 5 of an entry is set
    planar = network(40, 3, 1).model()
    assert len(planar['lut']) == 8 * 256 * 6 and any(planar['lut'][8 * 256 * 4:])


def test_cache_slots_follow_the_knob(check):
    for n, kb, slots in ((20, 0, 1024), (20, 4, 256), (20, 64, 4096), (256, 0, 128), (256, 1, 8), (100, 3, 64)):
        net = network(n, 2, n)
        got, want = lowered_net(check, net, cache_kb=kb), net.model(cache_kb=kb)
        assert want['head'][5] == slots
        for field in want:
            assert got[field] == want[field], (n, kb, field)


# ----------------------------------------------------------------------------- the problem space

class Space:
    def __init__(self, net, origin=0, any_nodes=(), fixed=(), fvar=(), sched=(), pvar=()):
        self.net, self.origin = net, origin
        self.any, self.fixed, self.fvar, self.sched, self.pvar = list(any_nodes), list(fixed), list(fvar), list(sched), list(pvar)

    def commands(self):
        flat = lambda entries: [v for e in entries for v in e]
        return [lst('origin', words(self.origin, self.net.w64, 64)), lst('any', self.any), lst('fixed', flat(self.fixed), 2),
                lst('fvar', flat(self.fvar), 2), lst('sched', flat(self.sched), 3), lst('pvar', flat(self.pvar), 3), 'space']

    def fixed_bits(self):
        values = {}
        for node, value in self.fixed:      # a later entry of a node wins
            values[node] = value
        return sum(1 << i for i in values), sum(v << i for i, v in values.items())

    def runs(self):
        """maximal runs of consecutive 'any' nodes inside one 32-bit word -> (first digit, word, shift, length)"""
        out = []
        for j, node in enumerate(self.any):
            if out and self.any[j - 1] == node - 1 and node % 32:
                out[-1][3] += 1
            else:
                out.append([j, node // 32, node % 32, 1])
        return out

    def model(self):
        n, nw = self.net.n, self.net.nw
        identity = self.any == list(range(len(self.any)))
        runs = [] if identity or len(self.any) > 64 or len(self.runs()) > MAX_RUNS else self.runs()
        tp_origin = max([0] + [t for t, _, _ in self.sched])
        dense = {}
        for t, node, value in self.sched:   # a later entry at the same (t, node) wins
            dense[t, node] = value
        set_bits, clr_bits = [0] * (tp_origin + 1), [0] * (tp_origin + 1)
        for (t, node), value in dense.items():
            (set_bits if value else clr_bits)[t] |= 1 << node
        variants = 1
        for rng in [r for _, r in self.fvar] + [r for _, _, r in self.pvar]:
            variants *= 3 if rng == ANY_Q else 2
        fixmask, fixval = self.fixed_bits()
        order = sorted(range(len(self.sched)), key=lambda j: (self.sched[j][0], j))     # stable by t
        return dict(head=[len(self.any), int(identity), len(runs), len(self.fvar), len(self.pvar), tp_origin,
                          max([tp_origin] + [t for t, _, _ in self.pvar]), min(variants, M64), int(variants > M64)],
                    origin=words(self.origin & ((1 << n) - 1) & ~sum(1 << a for a in self.any), MAX_W32),
                    fixmask=words(fixmask, MAX_W32), fixval=words(fixval, MAX_W32),
                    deposit=[v for src, word, shift, length in runs for v in (src | word << 8 | shift << 16, (1 << length) - 1)],
                    any=self.any, fv=[v for e in self.fvar for v in e], pv=[v for e in self.pvar for v in e],
                    set=[w for row in set_bits for w in words(row, nw)], clr=[w for row in clr_bits for w in words(row, nw)],
                    sched=[v for j in order for v in self.sched[j]])


SPACE_FIELDS = ['space', 'origin', 'fixmask', 'fixval', 'deposit', 'any', 'fv', 'pv', 'set', 'clr', 'sched']


def lowered_space(check, space, more=()):
    out = ask(check, space.net.commands() + space.commands() + list(more))
    out = out[len(NET_FIELDS):]
    if out[0][1] != '0':
        return failure(out[0], 'space')
    assert [l[0] for l in out[:len(SPACE_FIELDS)]] == SPACE_FIELDS
    got = {l[0]: ints(l, l[0]) for l in out[:len(SPACE_FIELDS)]}
    got['head'] = got.pop('space')[1:]
    got['more'] = out[len(SPACE_FIELDS):]
    return got


def plain_net(n):
    return Net(n, [[(i + 1) % n] for i in range(n)], [2] * n)


def check_space(check, space):
    got, want = lowered_space(check, space), space.model()
    for field in want:
        assert got[field] == want[field], field
    return want


def test_space_bits(check):
    for n in (1, 31, 33, 64, 65, 129, 200, 256):
        rng = random.Random(n)
        w64 = (n + 63) // 64
        picks = sorted(rng.sample(range(n), min(n, 7)))
        fixed = [(rng.randrange(n), rng.getrandbits(1)) for _ in range(5)]
        fixed += [(fixed[0][0], 1 - fixed[0][1]), (fixed[1][0], 1), (fixed[1][0], 0)]      # overwritten values
        want = check_space(check, Space(plain_net(n), origin=(1 << (64 * w64)) - 1, any_nodes=picks, fixed=fixed))
        # every bit at or above n and every 'any' bit is gone from the origin, all others are kept
        assert sum(w << (32 * j) for j, w in enumerate(want['origin'])) == ((1 << n) - 1) & ~sum(1 << a for a in picks)
        first = fixed[0][0]
        assert (want['fixval'][first // 32] >> (first % 32)) & 1 == ([v for node, v in fixed if node == first][-1])


def test_deposit_plan(check):
    net = plain_net(200)
    shapes = {'identity': list(range(30)), 'none': [], 'shifted': list(range(1, 31)),
              'across a word': list(range(28, 40)) + list(range(60, 70)) + [95, 96, 97, 130],
              'a whole word': list(range(32, 64)) + [64, 65], 'isolated, 64 runs': list(range(0, 128, 2)),
              'n_any 64, few runs': list(range(100, 164)), 'n_any 65': list(range(100, 165)),
              'identity of 65': list(range(65))}
    seen = {}
    for name, picks in shapes.items():
        want = check_space(check, Space(net, any_nodes=picks))
        seen[name] = want['head'][2]
    assert seen == {'identity': 0, 'none': 0, 'shifted': 1, 'across a word': 7, 'a whole word': 2, 'isolated, 64 runs': 64,
                    'n_any 64, few runs': 3, 'n_any 65': 0, 'identity of 65': 0}
    # (more than kMaxDepositRuns = 64 runs need more than 64 'any' nodes, for which there is no plan anyway)
    want = Space(net, any_nodes=shapes['a whole word']).model()
    assert want['deposit'][:2] == [0 | 1 << 8 | 0 << 16, M32] and want['deposit'][2:] == [32 | 2 << 8, 3]


def test_schedule_tables(check):
    net = plain_net(70)
    sched = [(5, 3, 1), (2, 69, 0), (5, 3, 0), (1, 40, 1), (2, 69, 1), (9, 0, 0), (5, 33, 1), (1, 40, 1), (5, 3, 1), (2, 5, 0)]
    pvar = [(3, 7, ANY_Q), (12, 1, 1), (1, 2, 2)]
    want = check_space(check, Space(net, any_nodes=[1, 2], fixed=[(4, 1)], fvar=[(6, 0), (4, ANY_Q)], sched=sched, pvar=pvar))
    nw = net.nw
    bit = lambda table, t, node: (want[table][t * nw + node // 32] >> (node % 32)) & 1
    assert (bit('set', 5, 3), bit('clr', 5, 3)) == (1, 0) and (bit('set', 2, 69), bit('clr', 2, 69)) == (1, 0)
    assert (bit('set', 9, 0), bit('clr', 9, 0)) == (0, 1) and len(want['set']) == 10 * nw
    assert [want['sched'][3 * j] for j in range(len(sched))] == sorted(t for t, _, _ in sched)
    assert want['sched'][6:15] == [2, 69, 0, 2, 69, 1, 2, 5, 0]                # equal times keep their order
    assert want['head'][5:7] == [9, 12]                                         # tp_origin, tp_max
    assert check_space(check, Space(net, sched=[(4, 1, 1)], pvar=[(2, 1, 0)]))['head'][5:7] == [4, 4]


def test_rejected_problem_spaces(check):
    def refused(**space):
        return lowered_space(check, Space(plain_net(12), **space))

    for bad in ([3, 2], [4, 4], [12], [0, 5, 40]):
        assert refused(any_nodes=bad) == (INVALID, "'any' nodes must be ascending node indices")
    for bad in ([(12, 0)], [(3, 2)], [(1, 1), (0, M32)]):
        assert refused(fixed=bad) == (INVALID, 'bad fixed node entry')
    for bad in ([(12, 0)], [(3, 4)], [(2, ANY_Q), (2, 77)]):
        assert refused(fvar=bad) == (INVALID, 'bad fixed-node variation')
    for bad in ([(0, 3, 1)], [(2, 12, 1)], [(2, 3, 2)]):
        assert refused(sched=[(1, 1, 1)] + bad) == (INVALID, 'bad perturbation entry')
    for bad in ([(0, 3, 1)], [(2, 12, 1)], [(2, 3, 4)]):
        assert refused(pvar=[(1, 1, ANY_Q)] + bad) == (INVALID, 'bad perturbation variation')
    # the checks run in the order any, fixed, fixed variations, schedule, perturbation variations, schedule length
    assert refused(any_nodes=[12], fixed=[(12, 0)])[1] == "'any' nodes must be ascending node indices"
    assert refused(fixed=[(12, 0)], fvar=[(12, 0)], sched=[(0, 0, 0)])[1] == 'bad fixed node entry'
    assert refused(sched=[(0, 0, 0)], pvar=[(0, 0, 0)])[1] == 'bad perturbation entry'
    too_long = (UNSUPPORTED, 'perturbation schedule too long for the dense table')
    assert refused(sched=[(1 << 27, 0, 1)]) == too_long and refused(sched=[(M32, 0, 1)]) == too_long    # (t + 1) * nw * 8 > 2^30
    assert refused(sched=[(1 << 27, 0, 1)], pvar=[(0, 0, 0)])[1] == 'bad perturbation variation'
    assert lowered_space(check, Space(plain_net(256), sched=[(1 << 24, 0, 1)])) == too_long


def test_variant_count_is_exact_up_to_2_64_minus_1_and_saturates_above(check):
    net = plain_net(64)
    for fvar, pvar in (([(j, ANY_Q) for j in range(40)], []),                                    # 3^40 < 2^64
                       ([(j, ANY_Q) for j in range(41)], []),                                    # 3^41 > 2^64
                       ([(j, 2) for j in range(40)], [(1 + j, j, 0) for j in range(23)]),        # 2^63
                       ([(j, 1) for j in range(40)], [(1 + j, j, 2) for j in range(24)]),        # 2^64: one too many
                       ([(j % 64, ANY_Q) for j in range(70)], [(3, 5, ANY_Q)] * 30),             # far above
                       ([(1, 0), (2, ANY_Q), (3, 2)], [(7, 1, ANY_Q), (2, 1, 1)])):              # 2 * 3 * 2 * 3 * 2
        want = check_space(check, Space(net, fvar=fvar, pvar=pvar))
        exact = 3 ** sum(r == ANY_Q for _, r in fvar) * 2 ** sum(r != ANY_Q for _, r in fvar)
        exact *= 3 ** sum(r == ANY_Q for _, _, r in pvar) * 2 ** sum(r != ANY_Q for _, _, r in pvar)
        assert want['head'][7:9] == ([exact, 0] if exact <= M64 else [M64, 1])
        assert want['head'][6] == max([0] + [t for t, _, _ in pvar])


# ----------------------------------------------------------------------------- problem indices

def index_tokens(digits, variant):
    return words(digits, 4, 64) + [variant]


def range_model(digits, variant, count, n_any, variants, saturated):
    if digits >> n_any:
        return INVALID, 'init_digits has bits at or above n_any'
    if not saturated and variant >= variants:
        return INVALID, 'variant number outside the problem space'
    if count:
        last_variant = variant + ((digits + count - 1) >> n_any)
        if last_variant > M64 or (not saturated and last_variant >= variants):
            return INVALID, 'first + count runs past the end of the problem space'
    return 0, ''


def test_range_check_against_python_integers(check):
    rng = random.Random(11)
    cases = []
    for n_any in (0, 1, 63, 64, 65, 255, 256):
        space = 1 << n_any
        for variants, saturated in ((1, 0), (5, 0), (M64, 0), (M64, 1)):
            for variant in sorted({0, variants - 1, min(variants, M64), min(variants + 1, M64)}):
                for digits in sorted({0, space - 1, space // 2, rng.randrange(space), space} - ({space} if n_any == 256 else set())):
                    left = (variants - variant) * space - digits        # problems from `first` to the end of the space
                    counts = {0, 1, 2, left - 1, left, left + 1, space - digits, space - digits + 1, 1 << 64, (1 << 64) + 1,
                              (1 << 128) - 1, rng.getrandbits(100)}
                    for count in sorted(c for c in counts if 0 <= c < 1 << 128):
                        cases.append((digits, variant, count, n_any, variants, saturated))
    out = ask(check, [cmd('range', *(index_tokens(d, v) + [c & M64, c >> 64, a, vc, s])) for d, v, c, a, vc, s in cases])
    want = [range_model(*case) for case in cases]
    got = [failure(l, 'range') for l in out]
    for case, g, w in zip(cases, got, want):
        assert g == w, case
    assert {w[1] for w in want} == {'', 'init_digits has bits at or above n_any', 'variant number outside the problem space',
                                    'first + count runs past the end of the problem space'}
    ok = [c for c, w in zip(cases, want) if w[0] == 0]
    assert any(c[2] >= 1 << 64 for c in ok) and any(c[5] and c[1] == M64 for c in ok)       # 2^64 and more; a saturated count
    # the last valid problem and the one past it
    assert range_model(0, 4, 1 << 65, 65, 5, 0)[0] == 0 and range_model(1, 4, 1 << 65, 65, 5, 0)[0] == INVALID


def test_index_plus_against_python_integers(check):
    rng = random.Random(12)
    cases = []
    for n_any in (0, 1, 63, 64, 65, 255, 256):
        space = 1 << n_any
        for _ in range(12):
            digits, variant = rng.randrange(space), rng.getrandbits(rng.choice((3, 40)))
            # a carry out of the digits, a whole number of variants, 2^64 and above, random
            for delta in (0, 1, space - digits, space - digits - 1 if digits + 1 < space else 0, 5 * space + 3,
                          min((1 << 128) - 1, space * rng.getrandbits(20) + rng.randrange(space)), rng.getrandbits(70) | 1 << 64):
                if n_any == 256:
                    delta = min(delta, space - 1 - digits)      # (nothing to carry into: stay inside the digits)
                if delta >> 128 or (digits + delta) >> n_any > M64 - variant:
                    continue
                cases.append((digits, variant, delta, n_any))
    out = ask(check, [cmd('plus', *(index_tokens(d, v) + [x & M64, x >> 64, a])) for d, v, x, a in cases])
    assert len(cases) > 300 and any(x >> 64 for _, _, x, _ in cases)
    for (digits, variant, delta, n_any), line in zip(cases, out):
        total = digits + delta
        assert ints(line, 'plus') == index_tokens(total % (1 << n_any), variant + (total >> n_any)), (digits, variant, delta, n_any)


# ----------------------------------------------------------------------------- target

def test_target_words(check):
    for w64 in (1, 2, 3, 4):
        rng = random.Random(w64)
        mask, code = rng.getrandbits(64 * w64) | 1 << (64 * w64 - 1), rng.getrandbits(64 * w64)
        out = ask(check, ['target {} {} {}'.format(hx(w64), ' '.join(map(hx, words(mask, w64, 64))), ' '.join(map(hx, words(code, w64, 64))))])
        assert ints(out[0], 'target') == words(mask, MAX_W32) + words(code, MAX_W32)


def test_variant_decoding_equals_problem_from_index(check):
    by_code = {code: rng for rng, code in RANGE_CODE.items()}
    assert by_code[ANY_Q] is NodeStateRange.MAYBE_TRUE_OR_FALSE
    n = 70
    fvar = [(3, 0), (40, 1), (69, 2), (5, ANY_Q), (40, ANY_Q), (33, 2), (64, 0), (3, 1)]       # all four ranges; nodes 3 and 40 twice
    fixed = [(3, 1), (7, 0), (33, 1), (66, 1)]
    radices = [3 if r == ANY_Q else 2 for _, r in fvar]
    n_variants = 1
    for r in radices:
        n_variants *= r
    variants = list(range(n_variants))
    space = Space(plain_net(n), fixed=fixed, fvar=fvar)
    got = lowered_space(check, space, more=[cmd('variant', v) for v in variants])
    assert got['head'][7] == n_variants == 2 ** 6 * 3 ** 2
    origin = ([False] * n, {node: bool(v) for node, v in fixed}, {})
    variations = ([], [(node, by_code[r]) for node, r in fvar], [])
    for v, line in zip(variants, got['more']):
        _, fixed_nodes, _ = batching.problem_from_index(v, origin, variations)
        want_mask, want_val = sum(1 << i for i in fixed_nodes), sum(1 << i for i, s in fixed_nodes.items() if s)
        assert ints(line, 'variant') == words(want_mask, MAX_W32) + words(want_val, MAX_W32), v


def test_cube_words_and_shares(check):
    rng = random.Random(5)
    cmds, want = [], []
    for _ in range(20):
        a, n_rel = rng.randrange(16, 64), rng.randrange(0, 14)
        umask, tmask, tcode = rng.getrandbits(256), rng.getrandbits(256) & rng.getrandbits(256), rng.getrandbits(256)
        cmds.append(cmd('cube', a, n_rel, *(words(umask, 8) + words(tmask, 8) + words(tcode, 8))))
        # the representative decides outside the irrelevant digits; inside them 2^-popcount of the members match at t = 0
        want.append([1 << n_rel, 1, a - n_rel, bin(tmask & umask).count('1')] + words(tmask & ~umask, 8) + words(tcode & tmask & ~umask, 8))
    shares = [(count, waves, chunk) for count in (1, 64, 65, 1000, (1 << 28) - 1, 1 << 28, 1 << 40) for waves, chunk in ((8, 64), (2048, 4096), (7, 128))]
    out = ask(check, cmds + [cmd('shares', *s) for s in shares])
    assert [ints(l, 'cube') for l in out[:20]] == want
    for (count, waves, chunk), line in zip(shares, out[20:]):
        assert ints(line, 'shares') == ([round_up(-(-count // waves), 64), 0] if count < 1 << 28 else [0, chunk])
    # listing pieces: what is left, but no more than max(2^16, 4 x the hits still wanted)
    pieces = [(left, wanted) for left in (1, 65535, 65536, 65537, 1 << 33) for wanted in (1, 16384, 16385, 1 << 31)]
    out = ask(check, [cmd('listing', *p) for p in pieces])
    assert [ints(l, 'listing')[0] for l in out] == [min(left, max(1 << 16, 4 * wanted)) for left, wanted in pieces]
    # cube passes: 16 <= n_any <= 64, identity or a run plan, no perturbations of any kind, a variant count that fits
    spaces = [(n_any, ident, runs, n_pv, tp, sat) for n_any in (15, 16, 64, 65) for ident, runs in ((1, 0), (0, 3), (0, 0))
              for n_pv, tp, sat in ((0, 0, 0), (1, 0, 0), (0, 2, 0), (0, 0, 1))]
    out = ask(check, [cmd('cubesok', *s) for s in spaces])
    assert [ints(l, 'cubesok')[0] for l in out] == [int(16 <= n_any <= 64 and (ident or runs) and not (n_pv or tp or sat))
                                                    for n_any, ident, runs, n_pv, tp, sat in spaces]


def count_plan(digit, variant, count, n_any, cubes):
    """The counted part of a summary call over `count` problems from (variant, digit) as a list of pieces:
    ('plain', at, n) and ('block', at, digit, a_bits, variant), `at` an offset into the call's range.  Inside every
    variant: a plain head up to the first multiple of 2^16, the body as aligned power-of-two blocks, each the largest
    that fits what is left of the body (at most 2^63), a plain tail; without cubes plain pieces of at most 2^32."""
    pieces, at = [], 0
    if not cubes:
        while at < count:
            pieces.append(('plain', at, min(count - at, 1 << 32)))
            at += pieces[-1][2]
        return pieces
    unit, space = 1 << CUBE_MIN_BITS, 1 << n_any
    while at < count:
        end = min(space, digit + count - at)            # this variant's segment is [digit, end)
        body, body_end = round_up(digit, unit), end // unit * unit
        if body >= body_end:
            pieces.append(('plain', at, end - digit))
        else:
            if body > digit:
                pieces.append(('plain', at, body - digit))
            d = body
            while d < body_end:
                a_bits = min(CUBE_MAX_BITS, n_any, (body_end - d).bit_length() - 1, (d & -d).bit_length() - 1 if d else CUBE_MAX_BITS)
                pieces.append(('block', at + d - digit, d, a_bits, variant))
                d += 1 << a_bits
            if end > body_end:
                pieces.append(('plain', at + body_end - digit, end - body_end))
        at += end - digit
        digit, variant = 0, variant + 1
    return pieces


def plan_cases():
    cases = []
    for n_any in (16, 17, 20, 64):
        space = 1 << n_any
        for digit, count in ((100, space - 100 + (1 << 16) + 5), (0, space), (0, 3 * space), (space - 3, 7), (5, 1000), (1 << 16, 1 << 16),
                             ((1 << 16) - 1, (1 << 16) + 2), (3 << 16, 3 * space), (space - (1 << 16) - 9, 2 * space + 20),
                             (space - (1 << 16) - 9, (1 << 17) + 100), (70000, 2 * space + 1)):
            cases.append((digit % space, 3, min(count, 1 << 40), n_any, 1))       # (a call takes at most 2^40 problems)
    cases += [(100, 0, (1 << 18) - 100 + (1 << 16) + 5, 18, 1), (0, 0, 1 << 40, 64, 1), (1 << 63, 2, 1 << 40, 64, 1)]
    cases += [(123, 1, c, 20, 0) for c in (1, 1 << 32, (1 << 32) + 1, (1 << 33) + 5, 1 << 40)]      # cubes off: above 2^32 in the plain branch
    return cases


def test_counting_plan(check):
    cases = plan_cases()
    out = ask(check, [cmd('plan', *c) for c in cases])
    for (digit, variant, count, n_any, cubes), line in zip(cases, out):
        flat = ints(line, 'plan')
        got, at = [], 0
        for n, block, d, a_bits, v in zip(*[iter(flat)] * 5):
            got.append(('block', at, d, a_bits, v) if block else ('plain', at, n))
            assert not block or n == 1 << a_bits
            # every piece begins in the variant it names ...
            assert not cubes or v == variant + ((digit + at) >> n_any)
            at += n
        assert at == count                                          # the pieces tile [0, count) in order
        assert got == count_plan(digit, variant, count, n_any, cubes), (digit, variant, count, n_any, cubes)
        for piece in got:
            if piece[0] == 'block':
                _, p_at, d, a_bits, v = piece
                size, space = 1 << a_bits, 1 << n_any
                assert CUBE_MIN_BITS <= a_bits <= CUBE_MAX_BITS and d % size == 0 and d + size <= space
                assert d == (digit + p_at) % space and v == variant + (digit + p_at) // space
                # ... lies inside the whole 2^16 units of its variant's part of the range ...
                seg_end = min(space, d + (count - p_at))
                assert d + size <= seg_end // (1 << 16) * (1 << 16)
                # ... and is the largest such block: twice the size is misaligned, runs past the body or exceeds 2^63
                assert a_bits == CUBE_MAX_BITS or a_bits == n_any or d % (2 * size) or d + 2 * size > seg_end // (1 << 16) * (1 << 16)
            else:
                assert cubes or piece[2] <= 1 << 32
    by_hand = count_plan(100, 0, (1 << 18) - 100 + (1 << 16) + 5, 18, 1)
    assert [p[0] for p in by_hand] == ['plain', 'block', 'block', 'block', 'plain']
    assert [p[3] for p in by_hand if p[0] == 'block'] == [16, 17, 16] and by_hand[3][4] == 1 and by_hand[4][2] == 5
    spans = {len({p[4] for p in count_plan(*c) if p[0] == 'block'}) for c in cases if c[4]}
    assert {0, 1, 2, 3} <= spans                                    # shorter than a block; one, two and three variants


# ----------------------------------------------------------------------------- simulate

def parent_sliced_ok(n, K, n_wide, n_fv, n_pv, knob, traj, final, digests, max_t, count):
    """bsx_run_simulate's own predicate before the unit existed (gen2_shape, sliced_ok)"""
    gen2_shape = K <= 3 and ((n + 15) & ~15) <= 128 and knob != 1
    return bool(knob != 0 and (final or digests) and not traj and (not digests or gen2_shape) and not n_fv and not n_pv and not n_wide and
                max_t >= 64 and max_t < STEP_LIMIT and count >= 2048 and ((n + 15) & ~15) * 136 * 4 <= 160 * 1024)


def parent_sliced_shape(n, K, knob, count, cus):
    """run_sim_sliced's launch shape before the unit existed"""
    rows = (n + 15) & ~15
    gen2 = K <= 3 and rows <= 128 and knob != 1
    shmem = rows * 1024 + (4096 + 64) * 4 if gen2 else (rows * (8 + 64) + max(rows, 32) * 64) * 4
    groups = (count + 4095) // 4096 if gen2 else (count + 2047) // 2048
    per_cu = 1 if gen2 else max(1, (160 * 1024) // shmem)
    return [int(gen2), rows, shmem, groups, per_cu, max(1, min(groups, cus * per_cu))]


def test_sliced_shape_and_predicate_agree_with_both_earlier_formulas(check):
    shapes = [(n, K, knob, count, cus) for n in (5, 16, 17, 128, 129, 256) for K in (1, 3, 4, 6) for knob in (-1, 1)
              for count, cus in ((2048, 256), (2049, 256), (1 << 20, 256), (1 << 30, 1), (4097, 3))]
    out = ask(check, [cmd('sliced', n, K, knob + 1, count, cus) for n, K, knob, count, cus in shapes])
    for shape, line in zip(shapes, out):
        assert ints(line, 'sliced') == parent_sliced_shape(*shape), shape
    assert [parent_sliced_shape(n, 1, -1, 2048, 1)[1] for n in (5, 16, 17, 128, 129)] == [16, 16, 32, 128, 144]
    assert parent_sliced_shape(16, 6, -1, 2048, 1)[2] == (16 * 72 + 32 * 64) * 4           # the max(rows, 32) term
    calls = [(n, K, n_wide, n_fv, n_pv, knob, traj, final, digests, max_t, count)
             for n in (5, 128, 129, 256) for K in (3, 4) for knob in (-1, 0, 1) for traj, final, digests in ((0, 1, 0), (0, 1, 1), (0, 0, 1), (1, 1, 0), (0, 0, 0))
             for n_wide, n_fv, n_pv in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)) for max_t, count in ((64, 2048), (63, 2048), (64, 2047), (STEP_LIMIT, 1 << 20), (STEP_LIMIT - 1, 1 << 20))]
    out = ask(check, [cmd('slicedok', n, K, nwd, nf, npv, knob + 1, *rest) for n, K, nwd, nf, npv, knob, *rest in calls])
    got = [ints(l, 'slicedok')[0] for l in out]
    assert got == [int(parent_sliced_ok(*c)) for c in calls] and 0 < sum(got) < len(got)
    for c, ok in zip(calls, got):
        # a call that wants digests is only sent to a launch that takes the second-generation kernel, the one that writes them
        if ok and c[8]:
            assert parent_sliced_shape(c[0], c[1], c[5], c[10], 256)[0] == 1
        # every admitted shape fits the LDS
        if ok:
            assert parent_sliced_shape(c[0], c[1], c[5], c[10], 256)[2] <= 160 * 1024
    counts = [(c, u) for c in (0, 1, 512, 513, 1 << 20, 1 << 40) for u in (1, 256)]
    out = ask(check, [cmd('simblocks', c, u) for c, u in counts])
    assert [ints(l, 'simblocks')[0] for l in out] == [max(1, min(4 * u, -(-c // BLOCK))) for c, u in counts]


def test_sliced_row_descriptors(check):
    for n in (5, 16, 17, 128, 129):
        for K in (1, 3, 6):
            if K > n:
                continue
            net = network(n, K, 7 * n + K)
            fixed = [(0, 1), (n - 1, 0), (n // 2, 1), (n // 2, 0)] if n > 2 else [(0, 1)]
            space = Space(net, fixed=fixed)
            got = lowered_space(check, space, more=[cmd('rowdesc', K)])
            desc = ints(got['more'][0], 'rowdesc')
            rows = round_up(n, 16)
            fixmask, fixval = space.fixed_bits()
            want = []
            for i in range(rows):
                row = [0] * 8
                if i < n:
                    k = len(net.preds[i])
                    row[:k] = net.preds[i]
                    if (fixmask >> i) & 1:
                        table = M64 if (fixval >> i) & 1 else 0                 # a constant rule
                    else:
                        table = sum(((net.tables[i] >> (idx % (1 << k))) & 1) << idx for idx in range(1 << K))
                    row[6], row[7] = table & M32, table >> 32
                want += row
            assert desc == want, (n, K)
            assert desc[6:8] == [M32, M32] and desc[8 * (n - 1) + 6:8 * (n - 1) + 8] == ([0, 0] if n > 2 else [M32, M32])
