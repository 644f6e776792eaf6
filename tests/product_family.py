"""
TEST INFRASTRUCTURE -- the product networks that pin the cube cascade at 2^48 .. 2^56 problems of 2^64 spaces (2^63 and 2^64
consecutive problems of a 2^96 space) against tests/product_ref.py, and the oracle sample of the north star that two tests share.

A member is a list of components (m nodes, K inputs per rule, seed: synth.random_network(m, K, seed)), a placement
(placement[c][j] = node of component c's bit j) and the calls the GPU test makes.  To the engine the text is one
ordinary network whose every node is 'any'.

What the selection had to respect (bsx_cascade.cpp: prepare_batch, lean_mirror_slots; DESIGN section 3 "Cycle-state
cache"): a block takes the cube path only while every cached attractor sits in the LDS mirror --
    at most kTagAcc + kLdsAcc = 64 attractors, every cycle of at most kCycleCacheMaxLen = 64 states, and
    4 x (sum of cycle states) <= cache_lds_slots: 1024 slots (n <= 32), 512 (n <= 64), 256 (n <= 128),
    so at most 256 / 128 / 64 joint cycle states.
Random component seeds multiply quickly (a product has prod(sum of the component's cycle lengths) joint cycle states),
so the seeds below were picked from a scan of seeds 100..399 by their cycle lengths and largest transient.  Per
component "seed: cycle lengths, largest mu" as product_ref.component finds them:

    K = 2, 16 nodes   100: [2, 2], 7     101: [5], 11    107: [2,2,2,2,10,10,10,10,20,20], 7    110: [2, 6], 5
                      115: [1], 10       116: [1], 15    117: [2], 10      152: [1], 9     159: [1], 11
                      172: [2], 15       242: [2], 29    347: [1], 21
    K = 3, 16 nodes   113: [1], 17     (163: [4], 36 and 116: [2, 2], 6 did not pass the sizing ladder, see below)
    K = 2, 22 nodes   123: [2, 6], 9     21 nodes   104: [2, 2], 22    121: [1], 15

tests/test_product_ref.py asserts these figures (attractors, cycle states, gcd splitting, proper lcm, mu >= 20, which
component supplies the largest mu in which block), so the table here cannot drift from the code.
"""
import functools
import random
from collections import namedtuple

from boolsi_amd import synth

import product_ref

Call = namedtuple('Call', 'first count max_t max_len env')
INF = float('inf')


def call(first, count, max_t=INF, max_len=INF, **env):
    return Call(first, count, max_t, max_len, tuple(sorted(env.items())))


def contiguous(sizes):
    out, at = [], 0
    for m in sizes:
        out.append(list(range(at, at + m)))
        at += m
    return out


def interleaved(n, k):
    """component = node index mod k"""
    return [list(range(c, n, k)) for c in range(k)]


class Member:
    def __init__(self, name, parts, placement, calls, top_log2):
        self.name, self.parts, self.placement, self.calls = name, parts, placement, calls
        self.n = sum(m for m, _, _ in parts)
        self.top_log2 = top_log2            # the largest aligned block the sizing ladder let this member keep

    @functools.lru_cache(maxsize=None)
    def components(self):
        return [product_ref.component(*synth.random_network(m, k, seed)) for m, k, seed in self.parts]

    def yaml(self):
        """The product as one network text: component nodes renamed to their placed names, every node 'any'."""
        rules = {}
        for (m, k, seed), nodes in zip(self.parts, self.placement):
            preds, masks = synth.random_network(m, k, seed)
            for j in range(m):
                rules[nodes[j]] = synth.rule_text([nodes[p] for p in preds[j]], masks[j])
        names = [synth.node_name(i) for i in range(self.n)]
        lines = ['nodes:'] + ['    - ' + v for v in names] + ['', 'update rules:']
        lines += ['    {}: {}'.format(names[i], rules[i]) for i in range(self.n)]
        lines += ['', 'initial state:'] + ['    {}: any'.format(v) for v in names]
        return '\n'.join(lines) + '\n'

    def table(self, c):
        return product_ref.product_table(self.components(), self.placement, c.first, c.first + c.count, c.max_t, c.max_len)

    def largest_mu_plus_lambda(self):
        comps = self.components()
        _, _, cycles = product_ref.joint_cycles(comps, self.placement)
        return max(c['max_mu'] for c in comps) + max(length for _, length in cycles)


def calls64(bases, top_log2, var_log2, cap_t, cap_log2):
    """The calls of an n = 64 member, cut at what the sizing ladder allowed: top_log2 = the largest aligned block that stayed
    under a second, var_log2 = the block that is run again under a cap, a length cap, forced sub-blocks and a forced depth.
    bases: three multiples of 2^48, one of them 0; cap_t: a max_t inside the transients."""
    unit = min(top_log2, 48)                                                   # 2^48, or the largest block the member keeps
    out = [call((b >> unit) << unit, 1 << unit) for b in bases]
    out += [call((1 << 56) - 12345, (1 << 20) + 24691),                        # odd ends across a 2^56 boundary
            call((0x2B << (unit + 2)) + 77777, (1 << (unit + 2)) + 99999)]     # about 2^50, from an odd index
    base = ((0xA5C3 << 48) >> var_log2) << var_log2
    out += [call(base, 1 << var_log2, INF, 1), call(base, 1 << var_log2, BSX_CUBE_SPLIT='1'), call(base, 1 << var_log2, BSX_CUBE_DEPTH='3')]
    if cap_t is not None:
        out += [call(((0xA5C3 << 48) >> cap_log2) << cap_log2, 1 << cap_log2, cap_t)]
    for big in (52, 56):
        if unit < big <= top_log2:
            out += [call(((0xA5C3 << 48) >> big) << big, 1 << big)]
    if top_log2 >= 63:
        out += [call(0, 1 << 63), call(1 << 63, 1 << 63)]
    if top_log2 >= 64:
        out += [call(0, 1 << 64)]
    return out


def scaled_calls(n, cap_t):
    """The analogous calls of a member whose whole space is 2^n problems, n = 32 or 48."""
    q = n - 16                                                                  # what 2^48 is to 2^64
    out = [call(0, 1 << q), call(0x5A5A << q, 1 << q), call(0xFFFF << q, 1 << q),
           call(0xA5 << (n - 8), 1 << (n - 8)), call(0, 1 << (n - 1)), call(1 << (n - 1), 1 << (n - 1)), call(0, 1 << n),
           call((1 << (n - 8)) - 12345, (1 << 20) + 24691), call((0x2B << (n - 14)) + 77777, (1 << (n - 14)) + 99999),
           call(0xA5 << (n - 8), 1 << (n - 8), cap_t), call(0xA5 << (n - 8), 1 << (n - 8), INF, 1),
           call(0xA5 << (n - 8), 1 << (n - 8), BSX_CUBE_SPLIT='1'), call(0xA5 << (n - 8), 1 << (n - 8), BSX_CUBE_DEPTH='3')]
    return out


def high_digit_calls(n, cap_t):
    """n = 96: more than 64 'any' nodes, so a call is cut at the multiples of 2^64 and the digits above belong to each
    stretch's origin state.  High digits non-zero everywhere but in the first call; one range crosses a multiple of 2^64."""
    hi = 0x9C3A5F17 << 64
    out = [call(0, 1 << 48), call(hi + (0xBEEF << 48), 1 << 48), call(hi + (0xA5 << 56), 1 << 56),
           call(hi, 1 << 63), call(hi, 1 << 64),
           call(hi + (1 << 64) - (1 << 50) - 4321, (1 << 51) + 99999),         # crosses (hi + 1) * 2^64 inside
           call((1 << n) - (1 << 56), 1 << 56),                                # the last block of the space
           call(hi + (0xA5 << 56), 1 << 56, INF, 1)]
    if cap_t is not None:
        out += [call(hi + (0xA5 << 56), 1 << 56, cap_t)]
    return out


# ---- the members --------------------------------------------------------------------------------------------------
# Joint figures (product_ref.joint_cycles), asserted in tests/test_product_ref.py::test_family_selection:
#   FOUR16   components 110, 101, 347, 242: cycle states 8 x 5 x 1 x 2 = 80; [2,6] x [2] splits every pair in two (gcd 2):
#            4 attractors, lengths 10, 10, 30, 30 (30 = lcm(6, 5, 2), longer than every component cycle); largest mu 29.
#            The top component (nodes 48..63) is seed 242: a 2^48 block whose top state has mu = 29 gets its largest mu
#            from that component, the block at 0 from another one.
#   UNEQUAL  22 + 21 + 21 nodes, seeds 123 ([2, 6], mu 9), 104 ([2, 2], mu 22), 121 ([1], mu 15): 32 cycle states, 8 attractors
#            (2, 2, 2, 2, 6, 6, 6, 6: every pair of cycles splits in two).
#   WITH_K3  K = 3 seed 113 ([1], mu 17) among K = 2 seeds 101, 117, 116: 10 cycle states, 1 attractor of length 10 (lcm(5, 2)).
#   N48      110, 101, 172: 80 cycle states, 4 attractors (10, 10, 30, 30).
#   N32      107, 117: 176 cycle states, 20 attractors (every cycle of 107 is even: gcd 2 with [2]).
#   N96      101, 117, 100, 116, 152, 159: 40 cycle states, 4 attractors of length 10.
FOUR16 = [(16, 2, 110), (16, 2, 101), (16, 2, 347), (16, 2, 242)]
UNEQUAL = [(22, 2, 123), (21, 2, 104), (21, 2, 121)]
WITH_K3 = [(16, 2, 101), (16, 2, 117), (16, 3, 113), (16, 2, 116)]
N48 = [(16, 2, 110), (16, 2, 101), (16, 2, 172)]
N32 = [(16, 2, 107), (16, 2, 117)]
N96 = [(16, 2, 101), (16, 2, 117), (16, 2, 100), (16, 2, 116), (16, 2, 152), (16, 2, 159)]


# name: (joint attractors, joint cycle states, longest joint cycle, largest mu)
FIGURES = {'four16': (4, 80, 30, 29), 'four16_interleaved': (4, 80, 30, 29), 'unequal': (8, 32, 6, 22), 'with_k3': (1, 10, 10, 17),
           'n48': (4, 80, 30, 15), 'n32': (20, 176, 20, 10), 'n96': (4, 40, 10, 15)}
# The cycle mirror holds cache_lds_slots / 4 joint cycle states (this file's header), by number of nodes.
MIRROR_STATES = {32: 256, 48: 128, 64: 128, 96: 64}
# CAP: the max_t of the capped call, inside the transients: between half of (largest mu + longest cycle) and that sum.  Half itself
# where the block then has many found and many not found; more for n96 and with_k3 (the joint mu is the largest of six / four, half
# finds nothing) and for four16, whose half, 29, lies below its longest cycle, 30 (see the notes below: such a call is exact but
# does not collapse).  The reference puts 14 % .. 86 % of the listed block on either side.
CAP = {'four16': 37, 'four16_interleaved': 37, 'unequal': 14, 'with_k3': 19, 'n48': 22, 'n32': 15, 'n96': 20}
# The capped call is listed at the largest block at which it stayed under 1000 ms on its own ladder (log2; notes below).
CAP_LOG2 = {'four16': 56, 'with_k3': 56, 'n48': 40, 'n32': 24, 'n96': 56}
CAPPED = tuple(CAP_LOG2)
# Contiguous FOUR16: a 2^48 block fixes the top component (seed 242).  Its state 0 has mu 9 (seed 347 then supplies the
# block's largest mu, 21), state 0x5e21 has mu 29 (the top component supplies it), state 0x94f1 lies on its cycle.
BASES_FOUR16 = (0, 0x5e21 << 48, 0x94f1 << 48)
BASES = (0, 0x3C96 << 48, 0xFFFF << 48)
# ---- the sizing ladder (one MI355X; aligned blocks, one process per rung under its own time limit, fresh engine + a 2^20
# discovery call, total_ms of the attract2 call; every rung that returned equalled product_table) ---------------------------------
#   member               2^32   2^40   2^48   2^52   2^56    beyond
#   four16               0.24   0.39   5.7    35     40      2^60: killed at its 150 s limit; nothing larger was tried after that
#   four16_interleaved   8.2    1.9    28     33     512     not tried (GPU time went to the rungs below)
#   unequal              1.4    8.0    189    62     986     not tried
#   with_k3, K = 3 seed 163 (first choice)   15   23   1762: over the line at 2^48, replaced
#            K = 3 seed 116 (1st replacement) 8.7  9.4  333    57     8819: reaches 2^52
#            K = 3 seed 113 (2nd replacement) 0.24 0.58 31     45     955: reaches 2^56, listed
#   n48                  0.22   0.23   24 (whole space; 2^47: 9.7)
#   n32                  0.36 (whole space)
#   n96                  9.1    9.4    11     --     40      2^60: 46, 2^63: 62, 2^64: 75
# Targets missed: no n = 64 member is listed beyond 2^56, so none reaches 2^63 or the whole 2^64; whole spaces are covered at
# n = 32 and 48, and 2^63 / 2^64 consecutive problems by stretches of the 2^96 space.
# The capped call, on a ladder of its own (same block bases as the listed calls):
#   four16, cap 37       0.24   0.27   5.7    28     32      listed at 2^56
#   four16, cap 29       --     --     --     --     75 s    exact, not listed: 29 is below the longest cycle (30)
#   with_k3, cap 19      --     --     31     56     960     listed at 2^56
#   n96, cap 20          9.5    9.0    12     35     46      listed at 2^56
#   unequal, cap 14      556    killed at 40 s (2^40), killed at 40 s (2^48): not listed
#   four16_interleaved, cap 29: killed at 390 s (2^56, first try) and at 40 s (2^52): not listed, not tried again
#   n48, cap 22 at 2^40: 0.06 s; n32, cap 15 at 2^24: 0.06 s
# What the reference says about the calls that did not return (an engine finding, VERDICT.md "Capped calls that do not collapse"):
#   * under cap 29 the two length-30 attractors of four16 can never be found (mu + 30 > 29), so they are never cached, the
#     71 % of the block that ends on them is never recognised by the cube passes, and the block falls back to halves and plain
#     enumeration; with cap 37 (both lengths can be found) the same block takes 32 ms;
#   * under cap 14 none of the first 2^20 problems of any block of unequal tried finds an attractor (reference: not found =
#     100 % there, 47 % .. 69 % over the block), so the discovery call caches nothing, the block takes no cube path
#     (dominant_launches = 0 at 2^32, 1.9e11 executed updates = plain enumeration) and 2^40 is 256 times that.
# The forced-depth call of unequal took 7.5 s at 2^52 and is listed at 2^48.
# Module on the GPU: 78 tests (77 calls and the north-star means) in about 9 s; most cases 0.05 .. 0.2 s, the slowest 1.8 s
# (four16 at 2^56 with forced sub-blocks), with_k3 at 2^56 and unequal's first case about 1 s each.
# Seeded errors, one run each against this list: sum_l2 shifted one bit less than count in merge_cube_counters turns 70 of the 78
# red (all but the seven max_len = 1 calls, whose tables are empty, and the north-star means); a mu = 0 correction booked with
# the wrong sign in the lower level turns 7 red (four16's 2^48 block on a cycle state of its top component, n48 at 2^47 (base 0)
# and 2^48, n32 at 2^31 twice and 2^32, the north-star means).  test_gpu_wide's every-variant-agrees test stays green under both.
# What the ladder left each n = 64 member (log2 of an aligned block): the largest block that stayed under 1000 ms, and the
# block that the length-capped / forced variants of the call use.
TOP_LOG2 = {'four16': 56, 'four16_interleaved': 56, 'unequal': 56, 'with_k3': 56}
VAR_LOG2 = {'four16': 56, 'four16_interleaved': 52, 'unequal': 48, 'with_k3': 52}


@functools.lru_cache(maxsize=None)
def members():
    def cap(name):
        return CAP[name] if name in CAPPED else None

    def m64(name, parts, placement, bases):
        return Member(name, tuple(parts), placement, calls64(bases, TOP_LOG2[name], VAR_LOG2[name], cap(name), CAP_LOG2.get(name)), TOP_LOG2[name])
    return (m64('four16', FOUR16, contiguous([16] * 4), BASES_FOUR16),
            m64('four16_interleaved', FOUR16, interleaved(64, 4), BASES),
            m64('unequal', UNEQUAL, contiguous([22, 21, 21]), BASES),
            m64('with_k3', WITH_K3, contiguous([16] * 4), BASES),
            Member('n48', tuple(N48), contiguous([16] * 3), scaled_calls(48, cap('n48')), 48),
            Member('n32', tuple(N32), contiguous([16] * 2), scaled_calls(32, cap('n32')), 32),
            Member('n96', tuple(N96), contiguous([16] * 6), high_digit_calls(96, cap('n96')), 64))


# ---- the north star, sampled by the oracle -------------------------------------------------------------------------

# key -> (cycle length, basin over all 2^64 initial states): tests/test_gpu_wide.py, profiles/r02_full_space.json, r03_full_space.json
NORTH_STAR = {0x19ac2dc3ba74bded: (16, 12076090139491696640), 0x19ac2dc3b875bd8f: (16, 6370653934217854976)}
NORTH_STAR_SAMPLES = 1 << 16


@functools.lru_cache(maxsize=None)
def north_star_sample():
    """2^16 problem indices drawn from random.Random(64).getrandbits(64), each through the CPU oracle on its own
    -> {key: (length, n, sum mu, sum mu^2)} and the number of samples without an attractor."""
    from boolsi_amd.compile import compile_problem
    from boolsi_amd.constants import Mode
    from boolsi_amd.input import parse_input_text
    from oracle.cpu_oracle import Oracle, key_int
    net, space = compile_problem(parse_input_text(synth.north_star_yaml(), 4096, Mode.ATTRACT))
    orc = Oracle(net, space)
    rng = random.Random(64)
    seen, lost = {}, 0
    for _ in range(NORTH_STAR_SAMPLES):
        pp, _, none, _ = orc.attract(rng.getrandbits(64), 1, 4096, cap=4)
        if none:
            lost += 1
            continue
        mu = int(pp['trajectory_l'][0])
        e = seen.setdefault(key_int(pp['key'][0]), [int(pp['length'][0]), 0, 0, 0])
        e[1] += 1
        e[2] += mu
        e[3] += mu * mu
    return {k: tuple(v) for k, v in seen.items()}, lost
