"""
The per-parent level's count (boolsi_amd/csrc/bsx_leaf.h) and its program (bsx_cube_plan.cpp: build_leaf_program) on the
CPU: tests/leaf_check.cpp is compiled with the host C++ compiler and no HIP include path and fed random programs --
kb 1-14, rules of 1-4 inputs with 1-4 added digits among them, random truth tables, parents and candidates, two and
four state words.  The unit's count must equal brute force over all 2^kb children, the per-part counts must add up to
it for every power-of-two split, and the program (digit numbering, the two rule lists, m) must be what the wiring says.
A second build with -fsanitize=address,undefined answers the same input identically.
"""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
hx = lambda v: format(int(v), 'x')
PROGRAMS, CASES_PER_PROGRAM = 320, 8


def build(tmp, extra=()):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp / 'leaf_check')
    csrc = os.path.join(ROOT, 'boolsi_amd', 'csrc')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', *extra, '-I' + os.path.join(ROOT, 'include'), '-I' + csrc,
                           os.path.join(ROOT, 'tests', 'leaf_check.cpp'), os.path.join(csrc, 'bsx_cube_plan.cpp'), '-o', exe])
    return exe


class Program:
    """A random network around kb added digits.  mode 0: every dependent rule reads one added digit; 1: the rules with
    several read a proper subset of the digits; 2: every digit is read together with another."""

    def __init__(self, rng, nw, kb, mode):
        self.nw, self.kb = nw, kb
        self.n = n = rng.randrange(max(kb + 8, 24), nw * 32 + 1)
        self.digit_nodes = rng.sample(range(n), kb)             # added digit p (child-index bit p) is this node
        others = [v for v in range(n) if v not in self.digit_nodes]
        self.any = self.digit_nodes + rng.sample(others, 3)
        rng.shuffle(self.any)
        self.added = [self.any.index(v) for v in self.digit_nodes]
        pool = {0: [], 1: rng.sample(range(kb), rng.randrange(2, kb)) if kb >= 3 else [], 2: list(range(kb)) if kb >= 2 else []}[mode]
        n_dep = rng.randrange(1, min(24, len(others), 3 + 2 * kb))
        dep_nodes = set(rng.sample(range(n), n_dep))
        chain = [(pool[i], pool[(i + 1) % len(pool)]) for i in range(0, len(pool), 2)]    # every digit of the pool gets a partner
        self.rules = []
        for i in range(n):
            if i not in dep_nodes:
                k = rng.randrange(0, 4)
                preds = rng.sample(others, k)
            else:
                k = rng.randrange(1, 5)
                if chain:
                    digits = list(chain.pop())
                    k = max(k, 2)
                    digits += rng.sample([q for q in pool if q not in digits], min(rng.randrange(0, k - 1), len(pool) - 2))
                else:
                    nd = rng.randrange(1, k + 1)
                    digits = rng.sample(pool, min(nd, len(pool))) if nd >= 2 and len(pool) >= 2 else [rng.randrange(kb)]
                preds = [self.digit_nodes[q] for q in digits] + rng.sample(others, k - len(digits))
                rng.shuffle(preds)
            self.rules.append((preds, rng.getrandbits(1 << len(preds))))
        self.fixed = set(rng.sample(sorted(dep_nodes), 1)) if rng.random() < 0.25 and n_dep > 2 else set()
        # ---- what the wiring says (the re-derivation build_leaf_program is checked against)
        pos = {v: p for p, v in enumerate(self.digit_nodes)}
        self.dep = []                                           # (node, set of digit positions)
        for i, (preds, _) in enumerate(self.rules):
            reads = {pos[v] for v in preds if v in pos}
            if reads and i not in self.fixed:
                self.dep.append((i, reads))
        entangled = set().union(*[r for _, r in self.dep if len(r) >= 2]) if self.dep else set()
        self.m = len(entangled)
        order = [p for p in range(kb) if p in entangled] + [p for p in range(kb) if p not in entangled]
        self.number = {p: q for q, p in enumerate(order)}       # digit position -> the program's number
        self.enum_rules = [i for i, r in self.dep if r & entangled]
        self.free_rules = sorted((self.number[min(r)], i) for i, r in self.dep if not (r & entangled))
        self.free_digit_rules = {}
        for q, i in self.free_rules:
            self.free_digit_rules.setdefault(q, []).append(i)

    def commands(self):
        fm = [0] * 8
        for i in self.fixed:
            fm[i >> 5] |= 1 << (i & 31)
        out = ['net {} {}'.format(hx(self.n), hx(self.nw))]
        out += ['node {} {} {} {}'.format(hx(i), hx(len(p)), ' '.join(hx(v) for v in p), hx(tt)).replace('  ', ' ') for i, (p, tt) in enumerate(self.rules)]
        out += ['fixmask ' + ' '.join(hx(w) for w in fm), 'fixval ' + ' '.join('0' for _ in fm)]
        out += ['any {} {}'.format(hx(len(self.any)), ' '.join(hx(v) for v in self.any))]
        out += ['program {} {}'.format(hx(self.kb), ' '.join(hx(v) for v in self.added))]
        return out

    def values(self, parent, children):
        """node -> the dependent rule's value for each child (numpy), children numbered by digit position"""
        pos = {v: p for p, v in enumerate(self.digit_nodes)}
        out = {}
        for i, _ in self.dep:
            preds, tt = self.rules[i]
            idx = np.zeros(len(children), dtype=np.int64)
            for j, v in enumerate(preds):
                bit = (children >> pos[v]) & 1 if v in pos else (parent >> v) & 1
                idx |= bit << j
            table = np.array([(tt >> x) & 1 for x in range(1 << len(preds))], dtype=np.int64)
            out[i] = table[idx]
        return out

    def brute(self, parent, cand):
        children = np.arange(1 << self.kb, dtype=np.int64)
        hit = np.ones(len(children), dtype=bool)
        vals = self.values(parent, children)
        for i, v in vals.items():
            hit &= v == ((cand >> i) & 1)
        # a free digit with no allowed value: none of its two values satisfies all of its rules (they read nothing else added)
        dead = False
        for q, rules in self.free_digit_rules.items():
            p = [p for p, qq in self.number.items() if qq == q][0]
            two = np.array([0, 1 << p], dtype=np.int64)
            v2 = self.values(parent, two)
            ok = [all(int(v2[i][x]) == ((cand >> i) & 1) for i in rules) for x in (0, 1)]
            dead = dead or not any(ok)
        return int(hit.sum()), dead


def words(v, nw):
    return ' '.join(hx((v >> (32 * w)) & 0xFFFFFFFF) for w in range(nw))


def generate():
    rng = random.Random(20260)
    progs = []
    for t in range(PROGRAMS):
        nw = (2, 4)[t & 1]
        mode = (t >> 1) % 3
        kb = rng.randrange(3 if mode == 1 else 2 if mode == 2 else 1, 15)
        P = Program(rng, nw, kb, mode)
        cases = []
        for c in range(CASES_PER_PROGRAM):
            parent = rng.getrandbits(32 * nw)
            cand = rng.getrandbits(32 * nw)
            if c % 2 == 0:                  # the first update of one of the children: at least that child hits
                child = np.array([rng.randrange(1 << kb)], dtype=np.int64)
                for i, v in P.values(parent, child).items():
                    cand = (cand & ~(1 << i)) | (int(v[0]) << i)
            cases.append((parent, cand))
        progs.append((P, cases))
    return progs


@pytest.fixture(scope='module')
def generated():
    return generate()


@pytest.fixture(scope='module')
def answers(tmp_path_factory, generated):
    lines = []
    for P, cases in generated:
        lines += P.commands()
        lines += ['count {} {} {}'.format(hx(P.nw), words(parent, P.nw), words(cand, P.nw)) for parent, cand in cases]
    text = '\n'.join(lines) + '\n'
    exe = build(tmp_path_factory.mktemp('leaf_check'))
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    return text, [l.split() for l in out.splitlines()]


def split_answers(generated, rows):
    """-> per program: (program line, digits line, rule lines, per case: (count, {parts: (per-part hits, children per part)}))"""
    it = iter(rows)
    out = []
    for P, cases in generated:
        head = next(it)
        assert head[0] == 'program' and head[1] == '1', head
        digits = next(it)
        n_rules = int(head[4], 16) + int(head[5], 16)
        rules = [next(it) for _ in range(n_rules)]
        m = int(head[3], 16)
        got = []
        for _ in cases:
            cnt = next(it)
            assert cnt[0] == 'count'
            splits = {}
            parts = 1
            while parts <= (1 << (m - 5) if m > 5 else 1):
                row = next(it)
                assert row[0] == 'parts' and int(row[1], 16) == parts and len(row) == 3 + parts
                splits[parts] = ([int(v, 16) for v in row[2:-1]], int(row[-1], 16))
                parts *= 2
            got.append((int(cnt[1], 16), splits))
        out.append((head, digits, rules, got))
    assert next(it, None) is None
    return out


def test_the_program_is_what_the_wiring_says(generated, answers):
    for (P, _), (head, digits, rules, _) in zip(generated, split_answers(generated, answers[1])):
        assert [int(v, 16) for v in head[2:]] == [P.kb, P.m, len(P.enum_rules), len(P.free_rules)]
        by_number = sorted(range(P.kb), key=lambda p: P.number[p])
        assert [int(v, 16) for v in digits[1:]] == [P.digit_nodes[p] for p in by_number]
        want_nodes = P.enum_rules + [i for _, i in P.free_rules]
        assert [int(r[1], 16) for r in rules] == want_nodes
        pos = {v: p for p, v in enumerate(P.digit_nodes)}
        for r, i in zip(rules, want_nodes):
            preds, tt = P.rules[i]
            assert int(r[2], 16) == len(preds) and int(r[4], 16) == tt
            assert [int(v, 16) for v in r[5:]] == [0x8000 | P.number[pos[v]] if v in pos else v for v in preds]
        assert [int(r[3], 16) for r in rules[len(P.enum_rules):]] == [q for q, _ in P.free_rules]
        assert all(q >= P.m for q, _ in P.free_rules)


def test_the_count_equals_brute_force_and_the_parts_add_up(generated, answers):
    n_cases = n_hits = n_dead = n_split = 0
    by_class = {'m = 0': 0, '0 < m < kb': 0, 'm = kb': 0}
    for (P, cases), (_, _, _, got) in zip(generated, split_answers(generated, answers[1])):
        for (parent, cand), (count, splits) in zip(cases, got):
            want, dead = P.brute(parent, cand)
            assert count == want, (P.kb, P.m, hx(parent), hx(cand))
            assert not (dead and want)
            for parts, (per_part, children) in splits.items():
                assert sum(per_part) == want and children * parts == 1 << P.kb and all(h <= children for h in per_part)
                n_split += parts > 1
            n_cases += 1
            n_hits += want != 0
            n_dead += dead
            by_class['m = 0' if P.m == 0 else 'm = kb' if P.m == P.kb else '0 < m < kb'] += 1
    print('cases {}, with hits {}, with a free digit without a value {}, splits into several parts {}, {}'.format(n_cases, n_hits, n_dead, n_split, by_class))
    assert n_cases >= 2000 and 4 * n_hits >= n_cases and n_dead >= 100 and n_split >= 100
    assert all(v >= 200 for v in by_class.values())


def test_the_sanitized_build_answers_the_same(tmp_path_factory, answers):
    text, rows = answers
    exe = build(tmp_path_factory.mktemp('leaf_check_san'), ('-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'))
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert [l.split() for l in run.stdout.splitlines()] == rows
