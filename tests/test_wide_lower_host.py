"""
boolsi_amd/csrc/bsx_wide_lower.cpp without a GPU: what the wide-state family's host side makes of a network and a
problem space before anything is uploaded -- row descriptors, the tables of the nodes with more than 6 predecessors,
fixed-variation slots, the sorted schedule, L, the variant count, the target words, the flat-index split, the grid.

tests/wide_lower_check.cpp is a stand-alone program that the host C++ compiler builds together with the unit, with no
HIP include path and -Wall -Wextra -Werror: that it builds this way is the proof that the unit does not depend on HIP.
It is built a second time with the address and undefined-behaviour sanitizers; each build runs as its own process.

The model below is written from the layout comments of bsx_wide.h, not from the unit:
  row i of `desc` (kWideDescWords = 8 words): words 0..2 the predecessors as u16 (input j in the low or high half of
  word j / 2), words 3..4 the 64-entry table replicated over the unused inputs, word 5 the fixed-variation slot or
  kWideNone, word 6 the index into wdesc or kWideNone; padding rows (n <= i < rows) are constant 0; an origin-fixed node
  is a constant rule with all predecessor fields 0; wdesc holds (k, first pred, first 32-bit table word) per node with
  more than 6 predecessors, in node order, fixed or not.
"""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
THREADS, BUFFERS, DESC_WORDS, MAX_W32 = 256, 4, 8, 32       # bsx_wide.h
MAX_PREDS, MAX_NODES_WIDE = 24, 1024                         # include/bsx.h
INVALID, UNSUPPORTED = -1, -4
ANY_Q = 3                                                    # BSX_RANGE_MAYBE_TRUE_OR_FALSE, radix 3

FLAGS = {'plain': [], 'sanitized': ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']}


@pytest.fixture(scope='module', params=list(FLAGS))
def check(request, tmp_path_factory):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('wide_lower_' + request.param) / 'wide_lower_check')
    csrc = os.path.join(ROOT, 'boolsi_amd', 'csrc')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror'] + FLAGS[request.param] +
                          ['-I' + os.path.join(ROOT, 'include'), '-I' + csrc, os.path.join(ROOT, 'tests', 'wide_lower_check.cpp'),
                           os.path.join(csrc, 'bsx_wide_lower.cpp'), '-o', exe])
    return exe


def ask(exe, lines):
    res = subprocess.run([exe], input='\n'.join(lines) + '\n', capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return [l.split() for l in res.stdout.splitlines()]


def hx(v):
    return format(v, 'x')


def split_words(value, n_words, bits):
    """an int as n_words little-endian words of `bits` bits (linear in its size, unlike shifting it word by word)"""
    raw = value.to_bytes(n_words * bits // 8, 'little')
    return [int.from_bytes(raw[at:at + bits // 8], 'little') for at in range(0, len(raw), bits // 8)]


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


# ----------------------------------------------------------------------------- cases and the model

class Case:
    """preds[i] ascending, tables[i] node i's whole truth table as an int; origin an int; the space as the ABI takes it"""

    def __init__(self, n, preds, tables, origin=0, any_nodes=(), fixed=(), fvar=(), sched=(), pvar=()):
        self.n, self.preds, self.tables, self.origin = n, preds, tables, origin
        self.any, self.fixed, self.fvar, self.sched, self.pvar = list(any_nodes), list(fixed), list(fvar), list(sched), list(pvar)
        self.rows, self.w64 = (n + 63) // 64 * 64, (n + 63) // 64

    def net_commands(self, po=None, tto=None, tt=None):
        po = po or [sum(len(p) for p in self.preds[:i]) for i in range(self.n + 1)]
        words = [max(1, (1 << len(p)) // 64) for p in self.preds]
        tto = tto or [sum(words[:i]) for i in range(self.n + 1)]
        tt = tt or [w for t, nw in zip(self.tables, words) for w in split_words(t, nw, 64)]
        return [lst('po', po), lst('pi', [p for ps in self.preds for p in ps]), lst('tto', tto), lst('tt', tt), 'net ' + hx(self.n)]

    def space_commands(self):
        flat = lambda entries: [v for e in entries for v in e]
        return [lst('origin', [(self.origin >> (64 * w)) & M64 for w in range(self.w64)]), lst('any', self.any),
                lst('fixed', flat(self.fixed), 2), lst('fvar', flat(self.fvar), 2), lst('sched', flat(self.sched), 3),
                lst('pvar', flat(self.pvar), 3), 'space']

    # -- the model
    def wide_nodes(self):
        return [i for i in range(self.n) if len(self.preds[i]) > 6]

    def net_model(self):
        wdesc, wpreds, wtt = [], [], []
        for i in self.wide_nodes():
            k = len(self.preds[i])
            wdesc += [k, len(wpreds), len(wtt)]
            wpreds += self.preds[i]
            wtt += split_words(self.tables[i], (1 << k) // 32, 32)
        K = max([1] + [len(p) for p in self.preds if len(p) <= 6])
        return dict(head=[self.n, self.rows, self.w64, K], wdesc=wdesc, wpreds=wpreds, wtt=wtt)

    def fixed_values(self):
        return {node: value for node, value in self.fixed}        # (a later entry of a node wins)

    def space_model(self):
        fixed = self.fixed_values()
        slot_of = {}
        fv = []
        for node, rng in self.fvar:
            fv += [node, rng, slot_of.setdefault(node, len(slot_of))]
        order = sorted(range(len(self.sched)), key=lambda j: (self.sched[j][0], j))     # stable by t
        origin = self.origin & ((1 << self.n) - 1) & ~sum(1 << a for a in self.any)
        desc = []
        wide_index = {node: at for at, node in enumerate(self.wide_nodes())}
        for i in range(self.rows):
            d = [0] * DESC_WORDS
            d[5] = d[6] = NONE
            if i < self.n:
                d[5] = slot_of.get(i, NONE)
                k = len(self.preds[i])
                if i in fixed:
                    d[3] = d[4] = M32 if fixed[i] else 0
                elif k > 6:
                    d[6] = wide_index[i]
                else:
                    for j, p in enumerate(self.preds[i]):
                        d[j // 2] |= p << (16 * (j % 2))
                    table = sum(((self.tables[i] >> (idx % (1 << k))) & 1) << idx for idx in range(64))
                    d[3], d[4] = table & M32, table >> 32
            desc += d
        variants = 1
        for _, rng in self.fvar:
            variants *= 3 if rng == ANY_Q else 2
        for _, _, rng in self.pvar:
            variants *= 3 if rng == ANY_Q else 2
        tp_origin = max([0] + [t for t, _, _ in self.sched])
        L, shmem = self.choose_l(len(slot_of), len(self.pvar))
        return dict(head=[len(slot_of), tp_origin, max([tp_origin] + [t for t, _, _ in self.pvar]), min(variants, M64),
                          int(variants > M64), L, shmem, len(self.any), len(self.fvar), len(self.pvar), len(self.sched)],
                    origin=[(origin >> (32 * w)) & M32 for w in range(MAX_W32)],
                    fixmask=[(sum(1 << i for i in fixed) >> (32 * w)) & M32 for w in range(MAX_W32)],
                    any=self.any, fv=fv, pv=[v for e in self.pvar for v in e], sched=[v for j in order for v in self.sched[j]],
                    desc=desc)

    def choose_l(self, n_fslots, n_pv):
        """the largest power of two in [4, 64] whose LDS words (wide_lds_words) fit 159 KiB; (0, 0): none"""
        for L in (64, 32, 16, 8, 4):
            words = BUFFERS * self.rows * L + 2 * (n_fslots + n_pv) * L + 2 * THREADS + 8 * L + 4 * 32 * L + 8
            if words * 4 <= 159 * 1024:
                return L, words * 4
        return 0, 0

    def step_direct(self, x):
        fixed = self.fixed_values()
        y = 0
        for i in range(self.n):
            if i in fixed:
                bit = fixed[i]
            else:
                idx = sum(((x >> p) & 1) << j for j, p in enumerate(self.preds[i]))
                bit = (self.tables[i] >> idx) & 1
            y |= bit << i
        return y


def step_by_descriptors(case, net, desc, x):
    """one update of state x as the kernel's rows evaluate it; padding rows included (they must stay 0)"""
    y = 0
    for i in range(case.rows):
        d = desc[DESC_WORDS * i:DESC_WORDS * (i + 1)]
        if d[6] != NONE:
            k, first_pred, first_word = net['wdesc'][3 * d[6]:3 * d[6] + 3]
            idx = sum(((x >> net['wpreds'][first_pred + j]) & 1) << j for j in range(k))
            bit = (net['wtt'][first_word + idx // 32] >> (idx % 32)) & 1
        else:
            idx = sum(((x >> ((d[j // 2] >> (16 * (j % 2))) & 0xFFFF)) & 1) << j for j in range(6))
            bit = ((d[3] | d[4] << 32) >> idx) & 1
        y |= bit << i
    return y


PRED_COUNTS = (0, 1, 6, 7, 2, 9, 3)        # per node in turn; node n / 2 takes `most` instead
MOST_AT = {65: MAX_PREDS}                   # (a table of 2^24 bits is 2^18 words to print and parse: one size carries it)


def network(n, seed):
    rng = random.Random(seed)
    preds = [sorted(rng.sample(range(n), min(PRED_COUNTS[i % len(PRED_COUNTS)], n))) for i in range(n)]
    if n >= 63:
        preds[n // 2] = sorted(rng.sample(range(n), MOST_AT.get(n, 12)))
    tables = [rng.getrandbits(1 << len(p)) for p in preds]
    return preds, tables


def bare_case(n):
    """no fixed nodes, no variations, no schedule: n_fslots = n_pv = 0"""
    preds, tables = network(n, 4000 + n)
    rng = random.Random(n)
    return Case(n, preds, tables, origin=rng.getrandbits(n), any_nodes=sorted(rng.sample(range(n), min(n, 5))))


def full_case(n):
    """every table of the space in use.  The first node with more than 6 predecessors is origin-fixed and an unfixed one
    follows; nodes a, b carry three fixed-node variations on two slots; the schedule is out of time order."""
    preds, tables = network(n, 5000 + n)
    rng = random.Random(7 * n)
    c = Case(n, preds, tables, origin=rng.getrandbits(n) | 1, any_nodes=sorted(rng.sample(range(n), min(n, 9))))
    wide = c.wide_nodes()
    if n >= 63:
        assert len(wide) >= 3 and n // 2 in wide
        c.fixed = [(wide[0], 1), (2, 0), (8, 1), (wide[-1], 0)]
    else:
        c.fixed = [(0, 1)]
    a, b = (n - 1, n // 3) if n > 1 else (0, 0)
    c.fvar = [(a, ANY_Q), (b, 0), (a, 2)] if n > 1 else [(0, 1), (0, ANY_Q)]
    pick = lambda: rng.randrange(n)
    c.sched = [(5, pick(), 1), (2, pick(), 0), (5, pick(), 0), (1, pick(), 1), (2, pick(), 1), (9, pick(), 0)]
    c.pvar = [(3, pick(), ANY_Q), (12, pick(), 1), (1, pick(), 2)]
    return c


SIZES = (1, 63, 64, 65, 257, 1024)
CASES = {'{}_{}'.format(kind.__name__[:4], n): kind(n) for n in SIZES for kind in (bare_case, full_case)}


LOWERED = {}


def lowered(check, case, name=None):
    """what the program makes of a case; the named cases are lowered once per build and shared by the tests"""
    if name and (check, name) in LOWERED:
        return LOWERED[check, name]
    out = ask(check, case.net_commands() + case.space_commands())
    assert [l[0] for l in out] == ['net', 'wdesc', 'wpreds', 'wtt', 'space', 'origin', 'fixmask', 'any', 'fv', 'pv', 'sched', 'desc']
    net = dict(head=ints(out[0], 'net')[1:], wdesc=ints(out[1], 'wdesc'), wpreds=ints(out[2], 'wpreds'), wtt=ints(out[3], 'wtt'))
    space = dict(head=ints(out[4], 'space')[1:], **{l[0]: ints(l, l[0]) for l in out[5:]})
    if name:
        LOWERED[check, name] = net, space
    return net, space


# ----------------------------------------------------------------------------- the tests

def test_case_mix():
    for name, c in CASES.items():
        assert c.rows % 64 == 0 and c.rows - 64 < c.n <= c.rows and c.w64 == c.rows // 64
        if c.n >= 63:       # K is the most inputs among the nodes with at most 6, not the most overall
            assert {0, 1, 6, 7, MOST_AT.get(c.n, 12)} <= {len(p) for p in c.preds} and c.net_model()['head'][3] == 6
    c = CASES['full_257']
    wide, fixed = c.wide_nodes(), c.fixed_values()
    assert wide[0] in fixed and wide[1] not in fixed                    # wide_at advances over the fixed node
    slots = [c.space_model()['fv'][3 * j + 2] for j in range(3)]
    assert slots == [0, 1, 0] and c.fvar[0][0] == c.fvar[2][0] != c.fvar[1][0]
    times = [t for t, _, _ in c.sched]
    assert times != sorted(times) and len(set(times)) < len(times)
    assert {c.space_model()['head'][5] for c in CASES.values()} >= {64, 32, 8}      # L differs with n


@pytest.mark.parametrize('name', list(CASES))
def test_lowered_arrays_equal_the_model(check, name):
    case = CASES[name]
    net, space = lowered(check, case, name)
    assert net == case.net_model()
    want = case.space_model()
    for field in want:
        assert space[field] == want[field], (name, field)
    assert want['head'][5] in (4, 8, 16, 32, 64)
    if name.startswith('full') and case.n >= 63:
        wide = case.wide_nodes()
        assert space['desc'][DESC_WORDS * wide[0] + 6] == NONE and space['desc'][DESC_WORDS * wide[1] + 6] == 1
        assert space['desc'][DESC_WORDS * wide[0]:DESC_WORDS * wide[0] + 5] == [0, 0, 0, M32, M32]


@pytest.mark.parametrize('name', list(CASES))
def test_one_step_by_the_descriptors_equals_the_truth_tables(check, name):
    case = CASES[name]
    net, space = lowered(check, case, name)
    rng = random.Random(name)
    states = [0, (1 << case.n) - 1] + [rng.getrandbits(case.n) for _ in range(30)]
    for x in states:
        assert step_by_descriptors(case, net, space['desc'], x) == case.step_direct(x), name


def test_variant_count_is_exact_up_to_2_64_minus_1_and_saturates_above(check):
    preds, tables = network(64, 1)
    for fvar, pvar in (([(j, ANY_Q) for j in range(40)], []),                                    # 3^40 < 2^64
                       ([(j, ANY_Q) for j in range(41)], []),                                    # 3^41 > 2^64
                       ([(j, 2) for j in range(40)], [(1 + j, j, 0) for j in range(23)]),        # 2^63
                       ([(j, 1) for j in range(40)], [(1 + j, j, 2) for j in range(24)]),        # 2^64: one too many
                       ([(j % 64, ANY_Q) for j in range(70)], [(3, 5, ANY_Q)] * 30)):            # far above
        case = Case(64, preds, tables, fvar=fvar, pvar=pvar)
        _, space = lowered(check, case)
        exact = 3 ** sum(r == ANY_Q for _, r in fvar) * 2 ** sum(r != ANY_Q for _, r in fvar)
        exact *= 3 ** sum(r == ANY_Q for _, _, r in pvar) * 2 ** sum(r != ANY_Q for _, _, r in pvar)
        assert space['head'][3:5] == ([exact, 0] if exact <= M64 else [M64, 1])
        assert space['head'] == case.space_model()['head']


def test_flat_index_split(check):
    rng = random.Random(3)
    cmds, want = [], []
    for n_any in (0, 1, 63, 64, 127, 128, 200):
        flats = [0, 1, M64, 1 << 64, (1 << 128) - 1] + [rng.getrandbits(rng.choice((20, 64, 100, 128))) for _ in range(12)]
        if n_any < 128:
            flats += [(M64 << n_any) & ((1 << 128) - 1), ((M64 << n_any) + (1 << n_any) - 1) & ((1 << 128) - 1)]
            if n_any < 64:
                flats += [1 << (64 + n_any), (1 << (64 + n_any)) - 1]
        for flat in flats:
            cmds.append('flat {} {} {}'.format(hx(flat & M64), hx(flat >> 64), hx(n_any)))
            digits, variant = (flat, 0) if n_any >= 128 else (flat & ((1 << n_any) - 1), flat >> n_any)
            if variant > M64:
                want.append((INVALID, 'first lies beyond the problem space'))
            else:
                want.append([0, digits & M64, digits >> 64, 0, 0, variant])
    out = ask(check, cmds)
    got = [failure(l, 'flat') if l[1] != '0' else ints(l, 'flat') for l in out]
    assert got == want
    assert sum(isinstance(w, tuple) for w in want) >= 6


def test_target_words(check):
    for n in (63, 65, 1024):
        case = Case(n, [[]] * n, [0] * n)
        rng = random.Random(n)
        mask, code = rng.getrandbits(case.w64 * 64), rng.getrandbits(case.w64 * 64)   # bits at or above n are dropped
        words = lambda v: [(v >> (64 * w)) & M64 for w in range(case.w64)]
        out = ask(check, case.net_commands() + ['target {} {} {}'.format(hx(case.w64), ' '.join(map(hx, words(mask))),
                                                                          ' '.join(map(hx, words(code))))])
        keep = (1 << n) - 1
        assert ints(out[-1], 'target') == [((v & keep) >> (32 * w)) & M32 for v in (mask, code) for w in range(MAX_W32)]


def test_grid_rule(check):
    """blocks = clamp(ceil(count / (32 L)), 1, CUs * max(1, 160 KiB / shmem))"""
    shapes = [(count, L, shmem, cus) for L in (4, 64) for shmem in (1024, 70000, 81920, 81921, 162816)
              for cus in (1, 256) for count in (0, 1, 32 * L, 32 * L + 1, 10 ** 6, 1 << 40)]
    out = ask(check, ['grid {} {} {} {}'.format(hx(c), hx(L), hx(s), hx(u)) for c, L, s, u in shapes])
    want = [max(1, min(-(-c // (32 * L)), u * max(1, (160 * 1024) // s))) for c, L, s, u in shapes]
    assert [ints(l, 'grid')[0] for l in out] == want


def small_net():
    """12 nodes: node 3 has inputs 1 < 4 < 9, node 5 has eight"""
    preds = [[(i + 1) % 12] for i in range(12)]
    preds[3], preds[5] = [1, 4, 9], [0, 1, 2, 3, 6, 7, 8, 11]
    return Case(12, preds, [random.Random(i).getrandbits(1 << len(p)) for i, p in enumerate(preds)])


def test_rejected_networks(check):
    c = small_net()
    po = [sum(len(p) for p in c.preds[:i]) for i in range(13)]
    tto = [sum(max(1, (1 << len(p)) // 64) for p in c.preds[:i]) for i in range(13)]

    def refused(case=c, **arrays):
        return failure(ask(check, case.net_commands(**arrays))[0], 'net')

    assert refused(po=po[:4] + [po[4] - 4] + po[5:]) == (INVALID, 'pred_offsets not monotone')
    c.preds[3] = [1, 4, 12]
    assert refused() == (INVALID, 'predecessor index out of range')
    c.preds[3] = [1, 9, 4]
    assert refused() == (INVALID, 'predecessors must be strictly ascending')
    c.preds[3] = [1, 4, 4]
    assert refused() == (INVALID, 'predecessors must be strictly ascending')
    c.preds[3] = [1, 4, 9]
    for node, delta in ((5, -1), (5, 1), (3, 1), (11, -1)):
        bad = tto[:node + 1] + [w + delta for w in tto[node + 1:]]
        assert refused(tto=bad) == (INVALID, 'truth table of a node must have ceil(2^k / 64) words')
    many = Case(40, [list(range(MAX_PREDS + 1))] + [[0]] * 39, [1] * 40)
    assert refused(many, tto=list(range(41)), tt=[1] * 40) == (UNSUPPORTED, 'node with more than BSX_MAX_PREDECESSORS predecessors')
    n = MAX_NODES_WIDE + 1
    assert refused(Case(n, [[]] * n, [0] * n)) == (UNSUPPORTED, 'more than BSX_MAX_NODES_WIDE nodes')
    assert ask(check, c.net_commands())[0][:2] == ['net', '0']                  # the unbroken network passes


def test_rejected_problem_spaces(check):
    def refused(n=12, **space):
        c = small_net()
        if n != 12:
            c = Case(n, [[]] * n, [0] * n)
        for name, value in space.items():
            setattr(c, name, value)
        return failure(ask(check, c.net_commands() + c.space_commands())[-1], 'space')

    for bad in ([3, 2], [4, 4], [12], [0, 5, 40]):
        assert refused(any=bad) == (INVALID, "'any' nodes must be ascending node indices")
    for bad in ([(12, 0)], [(3, 2)], [(1, 1), (0, M32)]):
        assert refused(fixed=bad) == (INVALID, 'bad fixed node entry')
    for bad in ([(12, 0)], [(3, 4)], [(2, ANY_Q), (2, 77)]):
        assert refused(fvar=bad) == (INVALID, 'bad fixed-node variation')
    for bad in ([(0, 3, 1)], [(2, 12, 1)], [(2, 3, 2)]):
        assert refused(sched=[(1, 1, 1)] + bad) == (INVALID, 'bad perturbation entry')
    for bad in ([(0, 3, 1)], [(2, 12, 1)], [(2, 3, 4)]):
        assert refused(pvar=[(1, 1, ANY_Q)] + bad) == (INVALID, 'bad perturbation variation')
    # the checks run in the order any, fixed, fixed variations, schedule, perturbation variations
    assert refused(any=[12], fixed=[(12, 0)])[1] == "'any' nodes must be ascending node indices"
    assert refused(fixed=[(12, 0)], fvar=[(12, 0)], sched=[(0, 0, 0)])[1] == 'bad fixed node entry'
    assert refused(sched=[(0, 0, 0)], pvar=[(0, 0, 0)])[1] == 'bad perturbation entry'
    # more tables per column than the LDS holds at L = 4 (the ABI stops at BSX_MAX_PERT_VARIATIONS; the unit has its own check)
    big = Case(1024, [[]] * 1024, [0] * 1024)
    assert big.choose_l(0, 2907) == (4, 159 * 1024) and big.choose_l(0, 2908) == (0, 0)
    assert lowered(check, Case(1024, [[]] * 1024, [0] * 1024, pvar=[(1, 0, 0)] * 2907))[1]['head'][5] == 4
    assert refused(n=1024, pvar=[(1, 0, 0)] * 2908) == (UNSUPPORTED, 'wide network: state matrices do not fit the LDS')
