"""
The family of tests/test_gpu_target_exact.py (target mode -- k_target, the hit compaction, bsx_run_target,
bsx_run_target_summary and its cube passes -- against the CPU oracle); tests/test_target_family.py proves on the CPU
what each member claims.  GPU-free.

A random target code on random nodes is mostly unreachable or reached at t = 0, so no member has one.  A target here
is the value, on a chosen node set, of the state s(t*) of a chosen problem p*, computed with Oracle.trajectory when
the member is built (what tools/make_config4.py does for config 4): p* certainly reaches it, by t* at the latest,
and its neighbours reach it at many different times.

A member has a name, a YAML text with the target state (text()), the max_t values to run, index ranges with the
shape each one claims, the histogram sizes of the summary, and two flags: cubes_expected (the aligned 2^16 blocks of
its ranges must go through cube passes) and at_cap (some problem first hits exactly at max_t and another one at
max_t + 1).
"""
import os
import random
from collections import namedtuple
from functools import lru_cache
from math import inf

import numpy as np

from boolsi_amd import synth
from boolsi_amd.compile import code_to_words, compile_problem
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text

CORES = min(16, len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1))

# shapes a range may claim (tests/test_target_family.py checks every claim):
#   'crosses'   a fixed-node / perturbation variant boundary lies strictly inside it
#   'unaligned' neither its first index nor its end is a multiple of 64 (the wave), let alone of 2^16
#   'edge'      its count is 4096 k + 1 or 4096 k - 1 (the compaction segment)
#   'block'     first is a multiple of 2^16 and the count one of 2^17: listing 5 hits leaves an aligned 2^16 block
Range = namedtuple('Range', 'first count claims')
HIST_BINS = (0, 1, 4, None, 2048)        # None: the largest first-hit time of the range + 2 (no clamp at all)


def network_text(preds, masks, initial=None, fixed=None, perturbations=None, target=None):
    """synth.network_yaml for explicit predecessor lists and truth tables (target: node -> '0' | '1', others any)"""
    n = len(preds)
    name = synth.node_name
    out = ['nodes:'] + ['    - ' + name(i) for i in range(n)] + ['', 'update rules:']
    out += ['    {}: {}'.format(name(i), synth.rule_text(preds[i], masks[i])) for i in range(n)]
    out += ['', 'initial state:'] + ['    {}: {}'.format(name(i), (initial or {}).get(i, 'any')) for i in range(n)]
    if fixed:
        out += ['', 'fixed nodes:'] + ["    {}: '{}'".format(name(i), s) for i, s in fixed.items()]
    if perturbations:
        out += ['', 'perturbations:']
        for i, by_state in perturbations.items():
            out.append('    {}:'.format(name(i)))
            out += ["        '{}': '{}'".format(s, times) for s, times in by_state.items()]
    if target is not None:
        out += ['', 'target state:'] + ['    {}: {}'.format(name(i), target.get(i, 'any')) for i in range(n)]
    return '\n'.join(out) + '\n'


def reached_target(make_text, p_star, t_star, nodes):
    """the values of `nodes` in s(t_star) of problem p_star of the space make_text(None) describes"""
    from oracle.cpu_oracle import Oracle
    net, space = compile_problem(parse_input_text(make_text(None), inf, Mode.SIMULATE))
    state = Oracle(net, space).trajectory(p_star, t_star)[t_star]
    return {i: str((int(state[i >> 6]) >> (i & 63)) & 1) for i in nodes}


class Member:
    def __init__(self, name, make_text, star, nodes, max_ts, ranges, cubes_expected=False, at_cap=False, lut_modes=(None,),
                 chain=None, reaches=''):
        """make_text(target or None) -> YAML; star = (p*, t*); nodes: the target node set; chain: (n, target mask,
        target code) of a shift network, which has a closed form; reaches: the untested paths this member is for"""
        self.name, self.make_text, self.star, self.nodes = name, make_text, star, list(nodes)
        self.max_ts, self.ranges = tuple(max_ts), [Range(*r) for r in ranges]
        self.cubes_expected, self.at_cap, self.lut_modes, self.chain, self.reaches = cubes_expected, at_cap, lut_modes, chain, reaches
        self.hist_bins = HIST_BINS
        self._compiled = None

    def __repr__(self):
        return self.name

    def text(self):
        return self.compiled()[0]

    def compiled(self):
        """-> (text, cfg, net, space, mask words, code words), built once"""
        if self._compiled is None:
            text = self.make_text(reached_target(self.make_text, self.star[0], self.star[1], self.nodes))
            cfg = parse_input_text(text, inf, Mode.TARGET)
            net, space = compile_problem(cfg)
            assert sorted(cfg['target node set']) == sorted(self.nodes)
            mask = code_to_words(sum(1 << i for i in cfg['target node set']), net.n_words)
            code = code_to_words(cfg['target substate code'], net.n_words)
            self._compiled = (text, cfg, net, space, mask, code)
        return self._compiled

    @lru_cache(maxsize=None)
    def reference(self, first, count, max_t):
        """The oracle over [first, first + count): (offsets of the reached problems, their first-hit times), read-only."""
        from oracle.cpu_oracle import Oracle
        _, _, net, space, mask, code = self.compiled()
        pp, _ = Oracle(net, space).target(first, count, max_t, mask, code, n_threads=CORES)
        off = np.nonzero(pp['reached'])[0].astype(np.uint64)
        t = pp['t_stop'][off.astype(np.int64)].astype(np.uint64)
        off.setflags(write=False)
        t.setflags(write=False)
        return off, t

    def closed_form(self, first, count, max_t):
        """Chain members: s(t) = (s(0) << t) masked to n bits, so the first hit needs neither oracle nor engine."""
        n, tmask, tcode = self.chain
        s = np.arange(first, first + count, dtype=np.uint64)
        t_hit = np.full(count, -1, dtype=np.int64)
        for t in range(int(min(max_t, n)) + 1):      # s(n) = 0 for good, and a target that asks for a 1 is not met by it
            hit = ((s & np.uint64(tmask)) == np.uint64(tcode)) & (t_hit < 0)
            t_hit[hit] = t
            s = (s << np.uint64(1)) & np.uint64((1 << n) - 1)
        off = np.nonzero(t_hit >= 0)[0]
        return off.astype(np.uint64), t_hit[off].astype(np.uint64)


def synth_member(name, n, k, seed, star, nodes, max_ts, ranges, any_nodes=None, fixed=None, perturbations=None, **kw):
    bits = synth.seeded_bits(n, seed + 1)
    initial = None if any_nodes is None else {i: str(bits[i]) for i in range(n) if i not in any_nodes}
    return Member(name, lambda target: synth.network_yaml(n, k, seed, initial=initial, fixed=fixed, perturbations=perturbations,
                                                          target=None if target is None else {i: target.get(i, 'any') for i in range(n)}),
                  star, nodes, max_ts, ranges, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# leaves: a 12-node K = 2 core that reads only itself (nodes 0-11) and 8 leaves that read the core and are read by
# nobody (nodes 12-19); all 20 nodes 'any'.  The digits of the leaves are irrelevant to the first update, four of them
# lie among the low 16 digits: every aligned 2^16 block has at least 4 irrelevant digits and must go through a cube pass.
N_CORE, N_LEAF = 12, 8


def sensitive_table(rng, k):
    while True:
        tt = rng.getrandbits(1 << k)
        if all(any(((tt >> x) ^ (tt >> (x ^ (1 << j)))) & 1 for x in range(1 << k)) for j in range(k)):
            return tt


def leaves_network(seed):
    rng = random.Random(seed)
    preds = [sorted(rng.sample(range(N_CORE), 2)) for _ in range(N_CORE + N_LEAF)]
    masks = [sensitive_table(rng, 2) for _ in range(N_CORE + N_LEAF)]
    return preds, masks


def leaves_member(name, seed, star, nodes, max_ts, ranges, knock_out=None, **kw):
    preds, masks = leaves_network(seed)
    fixed = {knock_out: '0?'} if knock_out is not None else None
    return Member(name, lambda target: network_text(preds, masks, fixed=fixed, target=target), star, nodes, max_ts, ranges,
                  cubes_expected=True, **kw)


def leaves_fixed_point(seed):
    """a state r = f(r) of leaves_network(seed) whose leaves among the low 16 digits (nodes 12-15) are all 0, or None"""
    preds, masks = leaves_network(seed)
    for core in range(1 << N_CORE):
        s = core
        for i in range(N_CORE, N_CORE + N_LEAF):
            s |= ((masks[i] >> (((core >> preds[i][0]) & 1) | ((core >> preds[i][1]) & 1) << 1)) & 1) << i
        nxt = 0
        for i in range(N_CORE + N_LEAF):
            nxt |= ((masks[i] >> (((s >> preds[i][0]) & 1) | ((s >> preds[i][1]) & 1) << 1)) & 1) << i
        if nxt == s and not (s >> N_CORE) & 0xF:
            return s
    return None


# ---------------------------------------------------------------------------------------------------------------------
# chain: x0' = 0, x_i' = x_(i-1), n = 20, all 'any'
N_CHAIN = 20


def chain_member(name, ones, max_ts, ranges, **kw):
    preds = [[]] + [[i - 1] for i in range(1, N_CHAIN)]
    masks = [0] + [0b10] * (N_CHAIN - 1)
    code = sum(1 << i for i in ones)
    # p* = the state with exactly the target's ones, t* = 0
    return Member(name, lambda target: network_text(preds, masks, target=target), (code, 0), ones, max_ts, ranges,
                  chain=(N_CHAIN, code, code), **kw)


K16, K17, K18 = 1 << 16, 1 << 17, 1 << 18
N40_ANY = [1, 2, 4, 7, 9, 12, 14, 17, 19, 22, 25, 27, 29, 31, 32, 34, 37, 39]
N100_ANY = [0, 3, 8, 13, 21, 30, 33, 41, 47, 52, 60, 64, 71, 77, 85, 93, 99]
N200_ANY = [2, 17, 31, 32, 50, 63, 64, 90, 111, 127, 128, 150, 166, 180, 192, 199]
N48_ANY = [0, 2, 3, 5, 8, 11, 13, 17, 21, 24, 28, 31, 32, 36, 40, 43, 45, 47]
N33_ANY = [0, 1, 3, 4, 6, 9, 11, 14, 18, 21, 25, 28, 31, 32]
LEAVES_PLAIN = [(0, K17, ('block',)), (3 * K16 - 4099, K17 + 8193, ('unaligned', 'edge'))]
# the '0?' knock-out doubles the space: variant 0 (no knock-out) is [0, 2^20), variant 1 is [2^20, 2^21)
LEAVES_KO = [((1 << 20) - K16 - 5, K17 + 10, ('crosses', 'unaligned')), (1 << 20, K17, ('block',))]
LEAVES_STAR = (35222, 2)
# leaves_network(40) has the fixed point r = 0x80ba1 whose leaves 12-15 are 0: in the block of r the class of r has a
# representative (irrelevant digits 0) that is r itself, f(r) = r, and every other member reaches r at t = 1
FIXED_POINT_SEED, FIXED_POINT = 40, 0x80BA1

FAMILY = [
    synth_member('n20_k2', 20, 2, 2020, (42450, 3), [0, 6, 8, 11, 12, 13], (inf, 6, 1),
                 [(0, K17, ('block',)), (K17 + 777, K16 + 4097, ('unaligned', 'edge'))], at_cap=True,
                 reaches='one state word; t == max_t and max_t + 1; compaction edges; BSX_ERR_TABLE_FULL; listing then counting'),
    synth_member('n40_k3_variants', 40, 3, 4037, (1331019, 4), [6, 7, 13, 14, 17, 18, 33, 38, 39], (inf, 5),
                 [(5 * K18 - 30011, K16 + 4095, ('crosses', 'unaligned', 'edge')), (8 * K18, K17, ('block',))],
                 any_nodes=N40_ANY, fixed={3: '0?', 35: 'any', 20: 'any?'}, at_cap=True,
                 reaches='mux class 3; 12 fixed-node variants, a range across a variant boundary (the skip carry); target on both sides of bit 32'),
    synth_member('n100_k2', 100, 2, 1023, (5423, 3), [36, 41, 48, 52, 53, 85, 93, 99], (300, 4),
                 [(0, K17, ('block',)), (4099, K16 - 1, ('unaligned', 'edge'))], any_nodes=N100_ANY, lut_modes=('0', '1', '2'),
                 reaches='four state words; LUT modes 0, 1 and 2; target in words 1, 2 and 3'),
    synth_member('n200_k4', 200, 4, 2004, (4924, 4), [22, 43, 113, 137, 140, 176, 192, 199], (100, 4),
                 [(0, K16, ()), (12345, 8193, ('unaligned', 'edge'))], any_nodes=N200_ANY, at_cap=True,
                 reaches='eight state words (NW = 8); mux class 4; target in words 0, 4 and 6; the last-bin clamp at 100 distinct times'),
    synth_member('n24_k9', 24, 9, 2416, (1104856, 3), [0, 2, 4, 6, 9, 18, 23], (200, 3),
                 [((1 << 20) + 5, K16 + 1, ('unaligned', 'edge')), (3 << 20, K16, ())], at_cap=True,
                 reaches='explicit-lookup rules (K > 6); 201 distinct first-hit times'),
    synth_member('n48_k6', 48, 6, 4806, (18250, 1), [8, 10, 13, 19, 23, 45], (100, 4),
                 [(0, K17, ('block',)), (K17 + 33, 4 * 4096 - 1, ('unaligned', 'edge'))], any_nodes=N48_ANY, at_cap=True,
                 reaches='the widest mux class (6); two state words'),
    # 14 'any' nodes x 3 x 2 perturbation variants; T_p is 7 or 9, so no hit is earlier than that
    synth_member('n33_perturbed', 33, 2, 3309, (35497, 2), [3, 19, 21, 23, 25, 27, 28, 32], (inf, 14),
                 [(0, 6 << 14, ('crosses',)), ((1 << 14) - 5001, K16 + 4097, ('crosses', 'unaligned', 'edge'))],
                 any_nodes=N33_ANY, perturbations={5: {'1': '2, 6-7', 'any?': '9'}, 30: {'0?': '3'}},
                 reaches='the warm-up phase under origin perturbations; perturbation variants across a boundary; a target node at bit 32'),
    leaves_member('leaves_leaf', 1, LEAVES_STAR, [12, 14, 19], (inf, 3), LEAVES_PLAIN, at_cap=True,
                  reaches='cube passes; t = 0 accounting with target nodes among the irrelevant digits only'),
    leaves_member('leaves_core', 1, LEAVES_STAR, [6, 7, 11], (inf, 3), LEAVES_PLAIN, at_cap=True,
                  reaches='cube passes; t = 0 accounting with target nodes among the relevant digits only'),
    leaves_member('leaves_both', 1, LEAVES_STAR, [6, 7, 12, 14], (inf, 3), LEAVES_PLAIN, at_cap=True,
                  reaches='cube passes; t = 0 accounting with target nodes among relevant and irrelevant digits'),
    leaves_member('leaves_knock_out', 1, ((1 << 20) + LEAVES_STAR[0], LEAVES_STAR[1]), [6, 7, 12, 14], (inf, 3), LEAVES_KO, knock_out=0, at_cap=True,
                  reaches='cube passes under a knock-out variant that changes which digits are relevant'),
    leaves_member('leaves_fixed_point', FIXED_POINT_SEED, (FIXED_POINT, 0), [4, 10, 12, 13], (inf, 3),
                  # the 2^16 block of r alone (irrelevant digits 12-15), then the 2^17 block around it (12-16; node 16 of r is 0 too)
                  [(FIXED_POINT & ~0xFFFF, K16, ()), (FIXED_POINT & ~0x1FFFF, K17, ('block',))],
                  reaches='a cube class whose representative is a fixed point that meets the target'),
    chain_member('chain_one', [9], (3, 1), [(0, K17, ('block',)), (4099, K16 + 4095, ('unaligned', 'edge'))], at_cap=True,
                 reaches='closed-form reference'),
    chain_member('chain_two', [7, 15], (inf, 3), [(0, K17, ('block',)), (4099, K16 + 4095, ('unaligned', 'edge'))], at_cap=True,
                 reaches='closed-form reference'),
]
BY_NAME = {mb.name: mb for mb in FAMILY}


# ---------------------------------------------------------------------------------------------------------------------
# seeded fuzz: 24 small cases with reached-state targets
N_FUZZ = 24
_STATES = ('0', '1', '0?', '1?', 'any', 'any?')


@lru_cache(maxsize=None)
def fuzz_member(seed):
    rng = random.Random(5000 + seed)
    n, k = rng.randint(16, 70), rng.randint(1, 4)
    n_any = rng.randint(12, min(n, 17))
    any_nodes = list(range(n_any)) if seed % 3 == 0 else sorted(rng.sample(range(n), n_any))
    fixed = {i: rng.choice(_STATES) for i in rng.sample(range(n), rng.randint(1, 2))} if seed % 2 else None
    pert = {rng.randrange(n): {rng.choice(('0', '1', '0?', 'any?')): '2, 4'}} if seed % 4 == 1 else None
    max_t = rng.choice((inf, 64, 8)) if (k == 1 or (k == 2 and n <= 40)) else rng.choice((64, 8))
    mb = synth_member('fuzz{}'.format(seed), n, k, 6000 + seed, None, rng.sample(range(n), rng.randint(3, 8)), (max_t,), [],
                      any_nodes=any_nodes, fixed=fixed, perturbations=pert)
    _, space = compile_problem(parse_input_text(mb.make_text(None), inf, Mode.SIMULATE))
    total = space.n_problems
    count = min(total, rng.randrange(1 << 12, K17 + 1))
    first = rng.randrange(0, total - count + 1)
    mb.star = (first + rng.randrange(count), rng.choice((2, 3, 4, 5, 8)))
    mb.ranges = [Range(first, count, ())]
    return mb
