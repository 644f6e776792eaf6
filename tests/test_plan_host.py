"""
The host arithmetic that the cube path's exactness rests on, checked without a GPU:

* the relevance analysis (bsx_cube_plan.cpp: build_cube, cube_levels) against a brute-force stepper over all
  members of a 2^10 block, the split planner's trees and choose_top against their defining properties;
* the unit accounting (bsx_merge.h: merge_cube_counters, fold_cube_level, book_unresolved_class, U256) against
  Python's integers.

tests/plan_check.cpp is compiled once per session with the host C++ compiler and no HIP include path: that it
builds this way is the proof that these units do not depend on HIP.

Semantics of the brute force (what the kernels do, bsx_kernels_common.h): s(0) = the origin's bits with the digits
deposited on the 'any' nodes; an update evaluates every rule on the previous state, an origin-fixed node takes its
fixed value instead; an origin perturbation (t, node, value) then overrides the node at time t.
"""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from boolsi_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, A, DEPTHS = 12, 10, 5
INF = (1 << 64) - 1
M128, M256 = (1 << 128) - 1, (1 << 256) - 1


@pytest.fixture(scope='session')
def plan_check(tmp_path_factory):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('plan_check') / 'plan_check')
    csrc = os.path.join(ROOT, 'boolsi_amd', 'csrc')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-I' + os.path.join(ROOT, 'include'), '-I' + csrc,
                           os.path.join(ROOT, 'tests', 'plan_check.cpp'), os.path.join(csrc, 'bsx_cube_plan.cpp'), '-o', exe])
    return exe


def ask(exe, lines):
    out = subprocess.run([exe], input='\n'.join(lines) + '\n', capture_output=True, text=True, check=True).stdout
    return [l.split() for l in out.splitlines()]


def hx(v):
    return format(v, 'x')


# ----------------------------------------------------------------------------- planner cases

class Case:
    """One block of 2^len(any) problems of a network; tables[i] is node i's whole truth table as an int."""

    def __init__(self, name, preds, tables, any_nodes, const=0, fixed=None, sched=(), fix_mask=0, fix_vals=0, n=N, n_block=None):
        self.name, self.n, self.preds, self.tables = name, n, preds, tables
        self.any, self.const, self.fixed, self.sched = list(any_nodes), const, dict(fixed or {}), list(sched)
        self.a = n_block if n_block is not None else len(self.any)
        self.fix_mask, self.fix_vals = fix_mask, fix_vals
        # digits at or above the block (d_lo) carry their share of the constants
        self.d_lo = sum(((const >> node) & 1) << j for j, node in enumerate(self.any) if j >= self.a)
        self.origin = const & ~sum(1 << node for node in self.any)

    def commands(self):
        words = lambda v: ' '.join(hx((v >> (32 * w)) & 0xFFFFFFFF) for w in range(8))
        out = ['net {} {}'.format(hx(self.n), hx(1 if self.n <= 32 else 2))]
        for i in range(self.n):
            out.append('node {} {} {} {}'.format(hx(i), hx(len(self.preds[i])), ' '.join(hx(p) for p in self.preds[i]),
                                                 hx(self.tables[i] & INF)))
        out.append('origin ' + words(self.origin))
        out.append('fixmask ' + words(sum(1 << i for i in self.fixed)))
        out.append('fixval ' + words(sum(v << i for i, v in self.fixed.items())))
        out.append('any {} {}'.format(hx(len(self.any)), ' '.join(hx(v) for v in self.any)))
        out.append('sched {} {}'.format(hx(len(self.sched)), ' '.join(hx(v) for e in sorted(self.sched) for v in e)))
        return out

    def members(self):
        x = np.arange(1 << self.a, dtype=np.int64)
        return x[(x & self.fix_mask) == self.fix_vals]

    def brute(self):
        """-> F[d][x] = state after d updates of block member x (every x of the 2^a, sub-block or not), d = 0 .. DEPTHS"""
        x = np.arange(1 << self.a, dtype=np.int64)
        s = np.full(x.shape, self.const & ~sum(1 << node for node in self.any[:self.a]), dtype=np.int64)
        for j, node in enumerate(self.any[:self.a]):
            s |= ((x >> j) & 1) << node
        F = [s]
        for d in range(1, DEPTHS + 1):
            nxt = np.zeros_like(s)
            for i in range(self.n):
                if i in self.fixed:
                    bit = np.full(s.shape, self.fixed[i], dtype=np.int64)
                else:
                    idx = np.zeros_like(s)
                    for j, p in enumerate(self.preds[i]):
                        idx |= ((s >> p) & 1) << j
                    table = np.array([(self.tables[i] >> r) & 1 for r in range(1 << len(self.preds[i]))], dtype=np.int64)
                    bit = table[idx]
                nxt |= bit << i
            for t, node, value in sorted(self.sched):
                if t == d:
                    nxt = (nxt & ~(1 << node)) | (value << node)
            s = nxt
            F.append(s)
        return F

    def exact_dependence(self, F):
        """-> per depth 1 .. DEPTHS the mask of free digits j with F^d(x) != F^d(x ^ 2^j) for some member x"""
        mem = self.members()
        out = []
        for d in range(1, DEPTHS + 1):
            mask = 0
            for j in range(self.a):
                if not (self.fix_mask >> j) & 1 and np.any(F[d][mem] != F[d][mem ^ (1 << j)]):
                    mask |= 1 << j
            out.append(mask)
        return out


def k2_network(seed):
    preds, masks = synth.random_network(N, 2, seed)
    return preds, masks


def planner_cases():
    plain, variants = [], []
    for seed in range(1, 25):
        preds, tables = k2_network(seed)
        rng = random.Random(1000 + seed)
        const = rng.getrandbits(2) << 10                  # nodes 10 and 11 are constant
        # (odd seeds: the constants sit in the origin; even seeds: nodes 10, 11 are 'any' too and d_lo holds them)
        any_nodes = list(range(10)) if seed & 1 else list(range(12))
        plain.append(Case('plain{}'.format(seed), preds, tables, any_nodes, const, n_block=A))
        if seed <= 6:                                     # 'any' nodes in another order than the nodes'
            order = rng.sample(range(N), N)
            variants.append(Case('order{}'.format(seed), preds, tables, order[:A], rng.getrandbits(N)))
        elif seed <= 12:                                  # one or two origin fixed nodes
            fixed = {node: rng.getrandbits(1) for node in rng.sample(range(N), 1 + seed % 2)}
            variants.append(Case('fixed{}'.format(seed), preds, tables, range(A), const, fixed=fixed))
        elif seed <= 18:                                  # origin perturbations at times 1 .. 3
            sched = {(rng.randint(1, 3), rng.randrange(N)): rng.getrandbits(1) for _ in range(1 + seed % 3)}
            variants.append(Case('pert{}'.format(seed), preds, tables, range(A), const, sched=[(t, nd, v) for (t, nd), v in sched.items()]))
        else:                                             # sub-blocks
            fix_mask = sum(1 << j for j in rng.sample(range(A), 1 + seed % 3))
            variants.append(Case('sub{}'.format(seed), preds, tables, range(A), const, fix_mask=fix_mask,
                                 fix_vals=rng.getrandbits(A) & fix_mask))
    rng = random.Random(77)
    # a rule with seven inputs: the analysis does not look into its table (conservative branch)
    preds, tables = k2_network(31)
    preds[3], tables[3] = sorted(rng.sample(range(N), 7)), rng.getrandbits(128)
    wide = Case('wide7', preds, tables, range(A), 1 << 11)
    # 1-input networks: node i copies node i + 1, node 11 keeps its value -- a digit is lost per update
    shift = Case('shift', [[min(i + 1, N - 1)] for i in range(N)], [0b10] * N, range(A), 1 << 10)
    # ... and a permutation with negations, one fixed node, one perturbation
    perm = rng.sample(range(N), N)
    permnet = Case('perm', [[p] for p in perm], [rng.choice((0b10, 0b01)) for _ in range(N)], range(A), 1 << 10,
                   fixed={perm[4]: 1}, sched=[(2, perm[7], 0)])
    return plain, variants, [wide, shift, permnet]


@pytest.fixture(scope='module')
def analysed(plan_check):
    """every planner case with the program's answer (ok, rel, levels) and the brute force (F, exact dependence)"""
    plain, variants, special = planner_cases()
    out = []
    for case in plain + variants + special:
        ans, = ask(plan_check, case.commands() + ['cube {} {} {} {} {}'.format(hx(case.d_lo), hx(case.a), hx(case.fix_mask), hx(case.fix_vals), hx(DEPTHS))])
        assert ans[0] == 'cube' and len(ans) == 3 + DEPTHS
        F = case.brute()
        out.append(dict(case=case, ok=int(ans[1]), rel=int(ans[2], 16), levels=[int(v, 16) for v in ans[3:]], F=F,
                        exact=case.exact_dependence(F)))
    return out


def test_case_mix():
    plain, variants, special = planner_cases()
    assert len(plain) == 24 and len(special) == 3
    for kind in ('order', 'fixed', 'pert', 'sub'):
        assert sum(c.name.startswith(kind) for c in variants) >= 6
    assert all(c.any != list(range(A)) for c in variants if c.name.startswith('order'))
    assert all(1 <= t <= 3 for c in variants for t, _, _ in c.sched)


def test_guard_blocks_do_collapse(analysed):
    """Not a vacuous run: by the brute force alone, the plain K = 2 blocks lose digits at depth 1 and more by depth 3."""
    plain = [r for r in analysed if r['case'].name.startswith('plain')]
    assert len(plain) == 24
    at1 = sum(bin(r['exact'][0]).count('1') < A for r in plain)
    at3 = sum(bin(r['exact'][2]).count('1') < bin(r['exact'][0]).count('1') for r in plain)
    print('guard: exact dependence below 10 digits at depth 1 in {} of 24 cases; smaller at depth 3 than at depth 1 in {}'.format(at1, at3))
    assert at1 >= 20 and at3 >= 12


def test_first_level_is_build_cubes_set_and_levels_nest(analysed):
    for r in analysed:
        assert r['ok'] == 1, r['case'].name
        assert r['levels'][0] == r['rel'], r['case'].name
        free = ((1 << r['case'].a) - 1) & ~r['case'].fix_mask
        assert r['rel'] & ~free == 0, r['case'].name
        for d in range(1, DEPTHS):
            assert r['levels'][d] & ~r['levels'][d - 1] == 0, (r['case'].name, d)


def test_sound_at_every_depth(analysed):
    """members that agree on the digits of R_d have the same F^d(x)"""
    for r in analysed:
        mem = r['case'].members()
        for d in range(1, DEPTHS + 1):
            classes = mem & r['levels'][d - 1]
            pairs = np.unique(np.stack([classes, r['F'][d][mem]]), axis=1).shape[1]
            assert pairs == np.unique(classes).size, (r['case'].name, d)
            assert r['exact'][d - 1] & ~r['levels'][d - 1] == 0, (r['case'].name, d)


def test_exact_at_depth_one(analysed):
    checked = 0
    for r in analysed:
        if max(len(p) for p in r['case'].preds) > 6:
            continue
        assert r['rel'] == r['exact'][0], r['case'].name
        checked += 1
    assert checked >= 50


def test_exact_at_every_depth_for_one_input_networks(analysed):
    by_name = {r['case'].name: r for r in analysed}
    for name in ('shift', 'perm'):
        assert by_name[name]['levels'] == by_name[name]['exact'], name
    assert [bin(l).count('1') for l in by_name['shift']['levels']] == [A - d for d in range(1, DEPTHS + 1)]


# ----------------------------------------------------------------------------- split trees, choose_top

SEEN = [[], ['seen {} {} {} {}'.format(which, hx(d), hx(4096 << d), hx(near))
             for which, fractions in ((0, (1, 3, 40, 300, 2000, 9000)), (1, (900, 700, 500, 300, 200, 100)))
             for d, near in enumerate(fractions, start=1)]]


def split_cases():
    plain, variants, special = planner_cases()
    cases = plain[:8] + [c for c in variants if not c.fix_mask][:6] + special
    for seed in range(1, 7):                  # blocks large enough for the estimate to split them unasked
        preds, tables = synth.random_network(48, 2, 100 + seed)
        cases.append(Case('big{}'.format(seed), preds, tables, range(44), n=48))
    return cases


def test_split_leaves_partition_the_block(plan_check):
    grown = []
    for case in split_cases():
        for seen in SEEN:
            for forced in (0, 1):
                ans, = ask(plan_check, case.commands() + ['seenclear'] + seen +
                           ['split {} {} {} {} 0'.format(hx(case.d_lo), hx(case.a), forced, hx(DEPTHS))])
                leaves = [tuple(int(v, 16) for v in l.split(':')) for l in ans[1:]]
                assert leaves, case.name
                block = (1 << case.a) - 1
                for mask, vals in leaves:
                    assert mask & ~block == 0 and vals & ~mask == 0, case.name
                for i, (m1, v1) in enumerate(leaves):
                    for m2, v2 in leaves[i + 1:]:
                        assert (v1 ^ v2) & m1 & m2, (case.name, 'two leaves share a member')
                assert sum(1 << (case.a - bin(mask).count('1')) for mask, _ in leaves) == 1 << case.a, case.name
                if forced:
                    assert len(leaves) <= 8
                grown.append((case.name, bool(seen), forced, len(leaves)))
    print('split trees (case, experience, forced, leaves):', grown)
    assert any(n > 1 for _, _, forced, n in grown if forced)


def test_choose_top_is_the_arg_min_of_the_estimate(plan_check):
    plain, variants, special = planner_cases()
    for case in plain[:12] + variants[::3] + special + split_cases()[-6:]:
        for seen in SEEN:
            for offered in range(1, DEPTHS + 1):
                for forced in (0, 1):
                    cmds = ['seenclear'] + seen + ['cube {} {} 0 0 {}'.format(hx(case.d_lo), hx(case.a), hx(offered)),
                                                  'top {} {} 0 0 {} {}'.format(hx(case.d_lo), hx(case.a), hx(offered), forced)]
                    cube, top = ask(plan_check, case.commands() + cmds)
                    costs = [float.fromhex(v) for v in top[3:]]
                    assert len(costs) == offered
                    key = [bin(int(v, 16)).count('1') for v in cube[3:]] if forced else costs   # (forced depth: fewest digits)
                    assert int(top[1], 16) == 1 + key.index(min(key)), (case.name, offered, forced)
                    assert float.fromhex(top[2]) == costs[int(top[1], 16) - 1]


# ----------------------------------------------------------------------------- the unit accounting

def signed(v):
    return v - (1 << 64) if v >> 63 else v


def edge_value(rng, top):
    """values near 2^49 and 2^64 as well as small and random ones, below 2^top"""
    v = rng.choice((0, 1, rng.getrandbits(8), (1 << 49) - rng.getrandbits(4), (1 << 49) + rng.getrandbits(4),
                    (1 << 64) - 1 - rng.getrandbits(4), rng.getrandbits(64)))
    return v & ((1 << top) - 1)


def two_complement(rng):
    return rng.choice((0, 1, -1, rng.getrandbits(20), -rng.getrandbits(20), (1 << 49) + 3, -(1 << 49) - 3, (1 << 62), -(1 << 62))) & INF


class Model:
    """bsx_merge.h in Python's integers (count: 128 bits, sums: 256 bits, as the library's types wrap)"""

    def __init__(self):
        self.table, self.none, self.ref = {}, 0, 0

    def slot(self, key, length):
        return self.table.setdefault(key, dict(length=length, count=0, sum_l=0, sum_l2=0))

    def counters(self, slots, sums, shift, max_t):
        for s in slots:
            if not s['acc_cnt'] and not s['fix_cnt']:
                continue
            e = self.slot(s['key'], s['len'])
            e['count'] = (e['count'] + (s['acc_cnt'] << shift) + signed(s['fix_cnt'])) & M128
            e['sum_l'] = (e['sum_l'] + (s['acc_sl'] << shift) + signed(s['fix_sl'])) & M256
            e['sum_l2'] = (e['sum_l2'] + ((s['acc_sl2_hi'] << 64 | s['acc_sl2_lo']) << shift) + signed(s['fix_sl2'])) & M256
        self.none = (self.none + (sums['n_none'] << shift) + signed(sums['fix_none'])) & M128
        self.ref = (self.ref + (sums['steps_ref'] << shift) + signed(sums['fix_ref']) +
                    (0 if max_t == INF else signed(sums['fix_capfail']) * max_t)) & M128

    def unresolved(self, members, t_class, shift, tp, cap_rel, max_t, max_len, key, lam, traj_l, found):
        m = (members << shift) & M128
        if not found:
            self.none = (self.none + m) & M128
            self.ref = (self.ref + m * max_t) & M128
            return True
        if traj_l == 0:
            return False
        mu = t_class + traj_l
        traj = tp + mu
        ok = cap_rel == INF or mu + lam <= cap_rel
        self.ref = (self.ref + (m * (traj + lam) if ok else m * max_t)) & M128
        if not ok or lam > max_len:
            self.none = (self.none + m) & M128
            return True
        e = self.slot(key, lam)
        e['count'] = (e['count'] + m) & M128
        e['sum_l'] = (e['sum_l'] + m * traj) & M256
        e['sum_l2'] = (e['sum_l2'] + m * (traj * traj & INF)) & M256
        return True


def key_words(rng, nw, pool):
    if pool and rng.random() < 0.6:
        return rng.choice(pool)
    key = tuple(rng.getrandbits(32) for _ in range(nw)) + (0,) * (8 - nw)
    pool.append(key)
    return key


@pytest.mark.parametrize('nw', [1, 2, 4, 8])
def test_merge_of_cube_counters_and_unresolved_classes(plan_check, nw):
    rng = random.Random(500 + nw)
    for max_t in (INF, 4096, (1 << 31) - 1):
        model, pool, cmds, booked = Model(), [], ['mreset'], []
        for shift in (0, 1, 31, 47, 63, 47, 0, 63):          # several blocks, the same keys arriving again
            slots = []
            for a in sorted(rng.sample(range(64), 5)):
                top = 128 - shift                             # (a count of 2^64 classes of 2^63 members is the ceiling)
                s = dict(slot=a, key=key_words(rng, nw, pool), len=rng.randint(1, 64), acc_cnt=edge_value(rng, min(64, top)),
                         acc_sl=edge_value(rng, 64), acc_sl2_lo=edge_value(rng, 64), acc_sl2_hi=edge_value(rng, 60),
                         fix_cnt=two_complement(rng), fix_sl=two_complement(rng), fix_sl2=two_complement(rng))
                for prev in slots:                            # (one attractor has one slot in a block)
                    if prev['key'] == s['key']:
                        s['key'] = key_words(rng, nw, [])
                known = model.table.get(s['key'])
                if known:
                    s['len'] = known['length']
                slots.append(s)
            slots[0]['acc_cnt'] = 0                           # a slot that only carries a correction
            slots[1]['acc_cnt'] = slots[1]['fix_cnt'] = 0     # ... and one that is skipped
            sums = dict(n_none=edge_value(rng, 64), steps_ref=edge_value(rng, 64), fix_none=two_complement(rng),
                        fix_ref=two_complement(rng), fix_capfail=two_complement(rng))
            cmds.append('ctr {} {} {}'.format(hx(nw), hx(shift), hx(max_t)))
            for s in slots:
                cmds.append('slot {} {} {} {}'.format(hx(s['slot']), ' '.join(hx(w) for w in s['key']), hx(s['len']), ' '.join(
                    hx(s[f]) for f in ('acc_cnt', 'acc_sl', 'acc_sl2_lo', 'acc_sl2_hi', 'fix_cnt', 'fix_sl', 'fix_sl2'))))
            cmds.append('sums ' + ' '.join(hx(sums[f]) for f in ('n_none', 'steps_ref', 'fix_none', 'fix_ref', 'fix_capfail')))
            cmds.append('end')
            model.counters(slots, sums, shift, max_t)
            # unresolved classes of that level: member counts up to 2^49 (in units of 2^shift problems)
            tp = rng.choice((0, 3))
            cap_rel = INF if max_t == INF else max_t - tp
            for _ in range(6):
                members = rng.choice((1, 5, (1 << 49) - 1, 1 << 49, rng.getrandbits(49)))
                t_class, traj_l, lam = rng.randint(0, 4), rng.choice((0, 1, 2, 900, 5000, (1 << 30))), rng.choice((1, 2, 7, 64, 200))
                found, max_len = int(rng.random() < 0.8), rng.choice((INF, 100))
                key = key_words(rng, nw, pool)
                if key in model.table:
                    lam = model.table[key]['length']
                state = [rng.getrandbits(32) for _ in range(nw)]
                cmds.append('unres {} {} {} {} {} {} {} {} {} {} {} {} {} {}'.format(
                    hx(nw), hx(shift), hx(tp), hx(cap_rel), hx(max_t), hx(max_len), ' '.join(hx(w) for w in state), hx(t_class),
                    hx(members & 0xFFFFFFFF), hx(members >> 32), ' '.join(hx(w) for w in key), hx(lam), hx(traj_l), hx(found)))
                booked.append(model.unresolved(members, t_class, shift, tp, cap_rel, max_t, max_len, key, lam, traj_l, found))
        out = ask(plan_check, cmds + ['mdump'])
        assert [int(l[1]) for l in out if l[0] == 'unres'] == [int(b) for b in booked]
        assert True in booked and False in booked
        recs = {}
        for l in out:
            if l[0] == 'rec':
                v = [int(x, 16) for x in l[1:]]
                key = tuple(w for k in v[0:4] for w in (k & 0xFFFFFFFF, k >> 32))
                recs[key] = dict(length=v[4], count=v[5] << 64 | v[6], sum_l=sum(w << (64 * i) for i, w in enumerate(v[7:11])),
                                 sum_l2=sum(w << (64 * i) for i, w in enumerate(v[11:15])))
        assert recs == model.table
        assert len(recs) >= 8 and any(e['count'] >> 64 for e in recs.values())
        sums = [int(x, 16) for x in out[-1][1:]]
        assert out[-1][0] == 'sums' and (sums[0] << 64 | sums[1], sums[2] << 64 | sums[3]) == (model.none, model.ref)


def test_u256_against_python_integers(plan_check):
    rng = random.Random(9)
    cmds, want = [], []
    words = lambda v: ' '.join(hx((v >> (64 * i)) & INF) for i in range(4))
    for _ in range(200):
        base = rng.getrandbits(rng.choice((0, 64, 130, 256)))
        lo, hi, shift = edge_value(rng, 64), edge_value(rng, 64), rng.choice((0, 1, 31, 47, 63, 64, 65, 127, rng.randrange(128)))
        cmds.append('ushift {} {} {} {}'.format(words(base), hx(lo), hx(hi), hx(shift)))
        want.append((base + ((hi << 64 | lo) << shift)) & M256)
        v = two_complement(rng)
        cmds.append('usigned {} {}'.format(words(base), hx(v)))
        want.append((base + signed(v)) & M256)
        a, b = rng.getrandbits(rng.choice((1, 49, 64, 112, 128))), edge_value(rng, 64)
        cmds.append('umul {} {} {} {}'.format(words(base), hx(a & INF), hx(a >> 64), hx(b)))
        want.append((base + a * b) & M256)
    got = [sum(int(w, 16) << (64 * i) for i, w in enumerate(l[1:])) for l in ask(plan_check, cmds)]
    assert got == want
