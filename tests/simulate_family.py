"""
The family of tests/test_gpu_simulate_exact.py (simulate mode -- k_simulate, k_simulate_sliced, k_simulate_sliced64,
bsx_run_simulate and its router, bsx_run_trajectories -- against the CPU oracle); tests/test_simulate_family.py proves on
the CPU what each member claims.  GPU-free.

A member has a name, a YAML text, the max_t values to run, index ranges with the shapes each one claims and the route
bsx_run_simulate takes on it when only final states are asked for ('per-lane', 'sliced' = k_simulate_sliced, 'sliced64' =
k_simulate_sliced64), and a `reaches` string that names the untested path it is for.  Per-lane members run about 700
problems (ragged against the 64-lane wave and the 512-thread workgroup, from an unaligned first index) and are compared
trajectory by trajectory; sliced members run 2048 + 37 to 4096 + 37 problems for 64 to 130 steps.

Two shapes of the kind one might ask for do not exist: a sliced run needs 2048 problems, and a network whose space has
them has at least 12 nodes (variations would add problems, but they keep a space off the sliced kernels), so the smallest
sliced member has n = 12 and n = 5 is a per-lane member; and a second pass of the sliced64 group loop needs more than
2^20 problems, hence n >= 21 and 32 rows, not 16.
"""
import os
import random
from collections import namedtuple
from functools import lru_cache
from math import inf

import numpy as np

from boolsi_amd import synth
from boolsi_amd.compile import CompiledSpace, compile_problem
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text
from target_family import network_text

CORES = min(16, len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1))

# shapes a range may claim (tests/test_simulate_family.py checks every claim):
#   'ragged'     its count is no multiple of 64 (the wave) nor of 512 (the per-lane workgroup), and on a sliced route no
#                multiple of 2048 (a sliced group) either
#   'unaligned'  its first index is no multiple of 64
#   'crosses'    a fixed-node / perturbation variant boundary lies strictly inside it
#   'tp_differs' two of its problems have different last perturbation times (the kernel's per-problem pr.tp)
Range = namedtuple('Range', 'first count claims route')
PER_LANE, SLICED, SLICED64 = 'per-lane', 'sliced', 'sliced64'
PLAIN = ('ragged', 'unaligned')
TrajList = namedtuple('TrajList', 'first offsets t_len')


def t_lens(tp_max):
    """the lengths a trajectory list draws from (tp_max: the member's last perturbation time)"""
    return (0, 1, tp_max - 1, tp_max, 200)


def without_schedule_entries(space, drop):
    """the space without the origin schedule rows for which drop(t, node, value) holds"""
    keep = [row for row in space.sched.tolist() if not drop(*row)]
    return CompiledSpace(n_nodes=space.n_nodes, origin_state=space.origin_state, any_nodes=space.any_nodes, fixed=space.fixed,
                         fixed_var=space.fixed_var, sched=np.array(keep, np.uint32).reshape(-1, 3), pert_var=space.pert_var,
                         n_problems=space.n_problems, radices=space.radices)


class Member:
    def __init__(self, name, text, max_ts, ranges, reaches, lut_modes=(None,), written=None, traj_list=None):
        """written: (predecessor lists, tables) as the text names them, where the member was not drawn by synth;
        traj_list: (first, offsets, t_len) for bsx_run_trajectories"""
        self.name, self.text, self.max_ts, self.reaches = name, text, tuple(max_ts), reaches
        self.ranges = [Range(*r) for r in ranges]
        self.lut_modes, self.written, self.traj_list = lut_modes, written, traj_list
        self._compiled = None

    def __repr__(self):
        return self.name

    @property
    def kind(self):
        return self.ranges[0].route

    def compiled(self):
        """-> (net, space), built once"""
        if self._compiled is None:
            self._compiled = compile_problem(parse_input_text(self.text, inf, Mode.SIMULATE))
        return self._compiled

    def oracle(self):
        from oracle.cpu_oracle import Oracle
        return Oracle(*self.compiled())

    def route(self, r, digest=False, knob=None):
        """the route of range r: with a digest sink; under BSX_SLICED = knob ('0' or '1')"""
        if knob == '0' or r.route == PER_LANE:
            return PER_LANE
        gen2 = r.route == SLICED64 and knob != '1'
        if digest and not gen2:
            return PER_LANE
        return SLICED64 if gen2 else SLICED

    @lru_cache(maxsize=None)
    def reference(self, first, count, max_t):
        """The oracle over [first, first + count): (final states (count, W), digests (count)), read-only."""
        _, final, digest, _ = self.oracle().simulate(first, count, max_t, want_traj=False, n_threads=CORES)
        final.setflags(write=False)
        digest.setflags(write=False)
        return final, digest

    def trajectories(self, first, count, max_t):
        """The oracle's whole trajectories (count, max_t + 1, W); not cached"""
        return self.oracle().simulate(first, count, max_t, want_traj=True, n_threads=CORES)[0]

    @lru_cache(maxsize=None)
    def trajectory(self, index, t_len):
        t = self.oracle().trajectory(index, t_len)
        t.setflags(write=False)
        return t


# seeds for which the oracle meets the conditions of tests/test_simulate_family.py, where the first one drawn did not
SEEDS = {'w31': 50001, 'w192': 50005, 'w193': 50005, 'k1_n40': 50006, 'g1_k2_n129': 50001, 'g2_n17_k1': 50002, 'g2_n17_k2': 50001,
         'g2_n112_k1': 50012, 'g2_n112_k2': 50004, 'g2_n113_k1': 50012, 'g2_n113_k2': 50003, 'g2_n128_k1': 50038, 'g2_n128_k2': 50001,
         'edges_g2_t64': 60002, 'edges_g2_t65': 60007, 'edges_lane_t40': 60114, 'edges_lane_t41': 60114}


def unaligned_first(n_any, salt):
    """an index inside a space of 2^n_any problems, no multiple of 64; in a large space one with high digits set"""
    if n_any <= 6:
        return 3
    small = 64 * (salt % 3 if n_any <= 12 else salt % 50 + 1) + 1 + 2 * (salt % 31)
    return small if n_any <= 20 else (1 << (n_any - 1)) + (1 << (n_any // 2)) + small


def synth_member(name, n, k, seed, max_ts, reaches, count=700, route=PER_LANE, fixed=None, perturbations=None, **kw):
    seed = SEEDS.get(name, seed)
    text = synth.network_yaml(n, k, seed, fixed=fixed, perturbations=perturbations)
    count = min(count, (1 << n) - unaligned_first(n, seed))
    return Member(name, text, max_ts, [(unaligned_first(n, seed), count, PLAIN, route)], reaches, **kw)


def some_wide_member(name, n, k, seed, max_ts, reaches):
    """every twelfth node reads k others, the rest three (the front end takes about a second per 12-input rule)"""
    rng = random.Random(SEEDS.get(name, seed))
    degrees = [k if i % 12 == 0 else 3 for i in range(n)]
    preds = [sorted(rng.sample(range(n), d)) for d in degrees]
    masks = [rng.getrandbits(1 << d) for d in degrees]
    return Member(name, network_text(preds, masks), max_ts, [(unaligned_first(n, seed), 700, PLAIN, PER_LANE)], reaches)


# ---------------------------------------------------------------------------------------------------------------------
# mixed: in-degrees 0 .. kmax by turns, predecessor lists written in drawn (unsorted) order, node 1 reads itself alone;
# `wide`: the last node reads 9 others
def mixed_network(n, kmax, seed, wide):
    rng = random.Random(seed)
    preds, masks = [], []
    for i in range(n):
        k = i % (kmax + 1)
        if wide and i == n - 1:
            k = 9
        p = rng.sample(range(n), k)
        if k >= 2 and p == sorted(p):
            p.reverse()
        if i == 1:
            p = [1]
        preds.append(p)
        masks.append(rng.getrandbits(1) if k == 0 else rng.randrange(1, (1 << (1 << k)) - 1))
    return preds, masks


def mixed_member(name, n, kmax, seed, wide, max_ts, count, route, reaches):
    seed = SEEDS.get(name, seed)
    preds, masks = mixed_network(n, kmax, seed, wide)
    return Member(name, network_text(preds, masks), max_ts, [(unaligned_first(n, seed), count, PLAIN, route)], reaches,
                  written=(preds, masks))


# ---------------------------------------------------------------------------------------------------------------------
# variations: 9 'any' nodes (512 problems per variant), three fixed-node variants (x 3 x 2 x 2) and two perturbation
# variants (x 2 x 3); the origin schedule ends at t = 7, the 'any?' perturbation, where a variant has it, at t = 25
VAR_TP = 25


def variations_text(n, seed, k=2):
    if n == 40:
        any_nodes, f, p = [1, 2, 4, 7, 9, 12, 14, 31, 32], (3, 17, 21), (5, 30)
    else:
        any_nodes, f, p = [1, 31, 32, 63, 64, 65, 101, 127, 128], (3, 77, 129), (5, 100)
    bits = synth.seeded_bits(n, seed + 1)
    initial = {i: str(bits[i]) for i in range(n) if i not in any_nodes}
    return synth.network_yaml(n, k, seed, initial=initial, fixed={f[0]: 'any?', f[1]: '0?', f[2]: 'any'},
                              perturbations={p[0]: {'1': '2, 6-7', 'any?': str(VAR_TP)}, p[1]: {'0?': '3'}})


# problem index = any digits (9 bits) + 512 * (fixed variant (12) + 12 * (the '0?' perturbation (2) + 2 * the 'any?' one (3)))
VAR_RANGES = [(512 * 24 - 333, 700, ('ragged', 'unaligned', 'crosses', 'tp_differs'), PER_LANE),
              (512 * 5 - 123, 700, ('ragged', 'unaligned', 'crosses'), PER_LANE),
              (512 * 48 - 401, 700, ('ragged', 'unaligned', 'crosses'), PER_LANE)]


def traj_list(seed, first, span, tp_max, n=700):
    """n offsets below span: unsorted, with repeats; lengths from t_lens(tp_max)"""
    rng = random.Random(seed)
    offsets = [rng.randrange(span) for _ in range(n - 40)]
    offsets += rng.sample(offsets, 40)                  # repeats
    rng.shuffle(offsets)
    t_len = [rng.choice(t_lens(tp_max)) for _ in range(n)]
    return TrajList(first, tuple(offsets), tuple(t_len))


# ---------------------------------------------------------------------------------------------------------------------
# perturbation edges: origin perturbations at t = 1 and t = max_t exactly, a run of consecutive times, two nodes at one
# time forced to both values, odd and even times; lo / hi: a node of the first and of the last eighth of the rows
def edges_member(name, n, k, seed, max_t, lo, hi, mid, count, route, reaches):
    seed = SEEDS.get(name, seed)
    perturbations = {lo: {'1': '1, 20', '0': '33'}, hi: {'0': '20, {}'.format(max_t), '1': '2'}, mid: {'1': '10-13'}}
    text = synth.network_yaml(n, k, seed, perturbations=perturbations)
    return Member(name, text, (max_t,), [(unaligned_first(n, seed), count, PLAIN, route)], reaches)


G1, G2 = 2048 + 37, 4096 + 37

WIDTHS = [synth_member('w{}'.format(n), n, 2, 100 + n, (40,), 'per-lane NW / w64 pairing at n = {}, all three sinks'.format(n))
          for n in (5, 31, 32, 33, 64, 65, 128, 129, 192, 193, 256)]
RULES = [synth_member('k{}_n40'.format(k), 40, k, 4000 + k, (40,), 'per-lane mux class {}'.format(k)) for k in range(1, 7)] + \
        [synth_member('k{}_n24'.format(k), 24, k, 2400 + k, (40,), 'wide rule ({} predecessors) in simulate'.format(k)) for k in (7, 9)] + \
        [some_wide_member('k12_n24', 24, 12, 2412, (40,), '12-input rules among mux-class ones in simulate')]
MIXED = [
    mixed_member('mixed9_n40', 40, 6, 4061, True, (40,), 700, PER_LANE, 'mixed in-degree 0-6 and a 9-input node, unsorted lists, a self-loop'),
    mixed_member('mixed9_n130', 130, 6, 1361, True, (40,), 700, PER_LANE, 'the same over five state words'),
    mixed_member('mixed06_n40', 40, 6, 4062, False, (64, 65), G1, SLICED, 'gen-1: table replicated over unused select inputs, in-degree 0-6'),
    mixed_member('mixed06_n130', 130, 6, 1362, False, (64,), G1, SLICED, 'gen-1: the same at 144 rows'),
    mixed_member('mixed03_n40', 40, 3, 4033, False, (64, 65), G2, SLICED64, 'gen-2: table replicated over unused select inputs, in-degree 0-3'),
]
VARIATIONS = [
    Member('var_n40', variations_text(40, SEEDS.get('var_n40', 77)), (40,), VAR_RANGES, 'per-problem tp, pv_digits, fm and fv in k_simulate'),
    Member('var_n130', variations_text(130, SEEDS.get('var_n130', 1377)), (40,), VAR_RANGES, 'the same with variation nodes in words 0, 2 and 4; scattered trajectories',
           traj_list=traj_list(130, 512 * 24 - 1333, 2700, VAR_TP)),
]
LUT = [synth_member('lut_n100', 100, 2, 1002, (40,), 'LUT modes 0, 1 and 2 with the trajectory sink', lut_modes=('0', '1', '2'))]
GEN1 = [
    synth_member('g1_k6_n40', 40, 6, 4606, (64, 65), 'gen-1 upper truth-table word (K = 6)', G1, SLICED),
    synth_member('g1_k4_n16', 16, 4, 1604, (64,), 'gen-1 at 16 rows: one batch per wave', G1, SLICED),
    synth_member('g1_k4_n17', 17, 4, 1704, (65,), 'gen-1 at 32 rows', G1, SLICED),
    synth_member('g1_k2_n129', 129, 2, 1292, (64,), 'gen-1 at the first n gen-2 refuses', G1, SLICED),
    synth_member('g1_k3_n256', 256, 3, 2563, (70,), 'gen-1 at 256 rows (139 KB of LDS)', G1, SLICED),
]
GEN2 = [synth_member('g2_n{}_k{}'.format(n, k), n, k, 10 * n + k, (64 + (n + k) % 2,), 'gen-2 at {} rows, K = {}'.format((n + 15) & ~15, k),
                     G2 if n > 12 else G1, SLICED64) for n in (12, 16, 17, 112, 113, 128) for k in (1, 2, 3)] + \
       [synth_member('g2_fixed_n40', 40, 3, 4035, (64, 65), 'gen-2 with a constant fixed 1 and a constant fixed 0 node', G2, SLICED64,
                     fixed={7: '1', 22: '0'})]
EDGES = [
    edges_member('edges_g2_t64', 128, 3, 1284, 64, 3, 125, 60, G2, SLICED64, 'gen-2 overrides: wave 0 and wave 15, t = 1 and t = max_t, both parities, even max_t'),
    edges_member('edges_g2_t65', 128, 3, 1285, 65, 6, 121, 61, G2, SLICED64, 'the same with an odd max_t'),
    edges_member('edges_g1_t64', 40, 5, 4054, 64, 3, 38, 17, G1, SLICED, 'gen-1 overrides at t = 1, t = max_t, both parities'),
    edges_member('edges_g1_t65', 40, 5, 4055, 65, 3, 38, 17, G1, SLICED, 'the same with an odd max_t'),
    edges_member('edges_lane_t40', 40, 2, 4052, 40, 3, 38, 17, 700, PER_LANE, 'per-lane overrides at t = 1 and t = max_t'),
    edges_member('edges_lane_t41', 40, 2, 4053, 41, 3, 38, 17, 700, PER_LANE, 'the same with an odd max_t'),
]
TRAJ_TP = 25


def _traj_member(name, n, k, seed, node):
    seed = SEEDS.get(name, seed)
    text = synth.network_yaml(n, k, seed, perturbations={node: {'1': '2, 6-7', '0': str(TRAJ_TP)}})
    first = unaligned_first(n, seed)
    return Member(name, text, (40,), [(first, 700, PLAIN, PER_LANE)], 'bsx_run_trajectories: scattered offsets, lengths below the last perturbation time',
                  traj_list=traj_list(seed, first, 3000, TRAJ_TP))


TRAJ = [_traj_member('traj_n33', 33, 2, 3302, 32), _traj_member('traj_n256', 256, 2, 2562, 200)]

FAMILY = WIDTHS + RULES + MIXED + VARIATIONS + LUT + GEN1 + GEN2 + EDGES + TRAJ
BY_NAME = {mb.name: mb for mb in FAMILY}
assert len(BY_NAME) == len(FAMILY)
TRAJ_MEMBERS = [mb for mb in FAMILY if mb.traj_list]

# second passes (tests/test_gpu_simulate_exact.py sizes the counts from the device): the networks alone
SECOND_PASS = {
    SLICED: synth.network_yaml(130, 2, 1302),
    SLICED64: synth.network_yaml(21, 2, 2102),
    PER_LANE: synth.network_yaml(20, 2, 2002),
}
