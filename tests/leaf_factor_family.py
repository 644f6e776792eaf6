"""
The network family of tests/test_gpu_leaf_factor.py (the per-parent level's factorised count: entangled digits enumerated,
free digits a factor; boolsi_amd/csrc/bsx_leaf.h); tests/test_leaf_factor_family.py proves on the CPU what each member
claims.

As tests/leaf_walk_family.py: a ring of R = 6 nodes that rotate, W layer-1 nodes that fall to 0, D layer-0 nodes whose
rules read layer-1 and ring nodes; nobody reads layer 0.  Here a member says for every layer-0 rule which layer-1 nodes it
reads (one: a single-digit rule; several: it entangles them) and how many ring nodes; the truth tables are random ones
that are sensitive to every input, written out as a disjunction of minterms, so they may be 1 where the layer-1 inputs
are 0.  A state on a cycle has layer 1 = 0 and layer 0 = what the rules give for layer 1 = 0 and the ring value before:
still one cycle state per ring value, one attractor per binary necklace, mu <= 2.  F^2 depends on the ring digits alone
and F^1 on the ring and layer-1 digits, so under a forced top depth of 2 the depth-1 level adds the W layer-1 digits
(kb = W) on top of 2^R parents, with the D layer-0 rules as its dependent rules.

The one cycle state that agrees with a parent's first update on the ring is the successor of the cycle state with the
parent's ring value, whose layer 1 is 0: the child with all added digits 0 always hits, so in this family no free digit
is ever left without an allowed value -- two rules on one digit contradict each other only about the value 1 (one allows
it, the other does not: factor 1) or agree (both allow it: factor 2).  The factor 0 is tests/test_leaf_factor_host.py's.
"""
import random

R = 6


class Member:
    def __init__(self, name, W, rules, m, pad_to=None):
        """rules: (layer-1 digits read, ring nodes read) per layer-0 rule; m: the entangled digits it claims"""
        self.name, self.W, self.rules, self.m = name, W, list(rules), m
        if pad_to:                      # more single-digit rules on the free digits: n = pad_to, m unchanged
            entangled = set().union(*[set(d) for d, _ in self.rules if len(d) > 1])
            free = [q for q in range(W) if q not in entangled]
            j = 0
            while R + W + len(self.rules) < pad_to:
                self.rules.append(((free[j % len(free)],), 1 + j % 3))
                j += 1
        self.D = len(self.rules)
        self.n = R + W + self.D

    def tables(self):
        """per rule: (input names, truth table over them, bit idx = output when input j is (idx >> j) & 1)"""
        rng = random.Random(7000 + 100 * self.W + self.D)
        out = []
        for digits, n_ring in self.rules:
            names = ['a{}'.format(q) for q in digits] + ['r{}'.format(i) for i in rng.sample(range(R), n_ring)]
            k = len(names)
            while True:
                tt = rng.getrandbits(1 << k)
                if all(any(((tt >> x) ^ (tt >> (x ^ (1 << j)))) & 1 for x in range(1 << k)) for j in range(k)):
                    break
            out.append((names, tt))
        return out

    def yaml(self):
        ring = ['r{}'.format(i) for i in range(R)]
        lay1 = ['a{}'.format(i) for i in range(self.W)]
        lay0 = ['d{}'.format(i) for i in range(self.D)]
        rules = {v: ring[(i + 1) % R] for i, v in enumerate(ring)}
        rules.update({v: 'r0 and not r0' for v in lay1})
        for v, (names, tt) in zip(lay0, self.tables()):
            terms = [' and '.join(('' if (x >> j) & 1 else 'not ') + nm for j, nm in enumerate(names)) for x in range(1 << len(names)) if (tt >> x) & 1]
            rules[v] = ' or '.join('({})'.format(t) for t in terms)
        names = ring + lay1 + lay0
        lines = ['nodes:'] + ['    - ' + v for v in names] + ['', 'update rules:']
        lines += ['    {}: {}'.format(v, rules[v]) for v in names]
        lines += ['', 'initial state:'] + ['    {}: any'.format(v) for v in names]
        return '\n'.join(lines) + '\n'


def pairs(*ds):
    return [(d, 1) for d in ds]


def singles(qs, n_ring=1):
    return [((q,), n_ring) for q in qs]


FAMILY = [
    # three digits carry two free rules each: about the value 1 they contradict for some ring values and agree for others
    Member('kb10_m0', 10, singles(range(10)) + singles((0, 1, 2), 2), 0),
    Member('kb9_m2', 9, pairs((0, 1)) + singles(range(2, 9)) + singles((0,), 2), 2),
    # the bench's shape: four rules with two added digits, six entangled digits
    Member('kb12_m6', 12, pairs((0, 1), (2, 3), (4, 5), (1, 2)) + singles(range(6, 12)) + singles((3, 7), 2), 6),
    # everything entangled: today's path, two pieces of 512 children
    Member('kb10_m10', 10, pairs((0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (1, 2), (5, 6), (0, 9)) + singles((3, 7)), 10),
    # four pieces, parts of one word and more, on 64 parents
    Member('kb13_m11', 13, pairs((0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (9, 10), (1, 2, 3)) + singles((11, 12), 2), 11),
    # fewer children than a word (more single-digit rules on the free digits make the space large enough for a block)
    Member('kb3_m0', 3, singles(range(3)) + singles((1,), 2), 0, pad_to=20),
    Member('kb4_m3', 4, pairs((0, 1, 2)) + singles((3, 0)), 3, pad_to=20),
    # rules of three and four inputs, with one and with three added digits
    Member('kb8_m5', 8, [((0, 1, 2), 1), ((2, 3, 4), 0), ((5,), 2), ((6,), 3), ((7,), 1), ((5,), 3), ((0,), 2)], 5),
]
BY_NAME = {mb.name: mb for mb in FAMILY}
# the m = 6 member padded to two and to four state words
WIDE = [Member('kb12_m6_n49', 12, BY_NAME['kb12_m6'].rules, 6, pad_to=49), Member('kb12_m6_n80', 12, BY_NAME['kb12_m6'].rules, 6, pad_to=80)]


def necklaces(ring):
    out = {}
    for v in range(1 << ring):
        orbit = {((v >> r) | (v << (ring - r))) & ((1 << ring) - 1) for r in range(ring)}
        out.setdefault(min(orbit), len(orbit))
    return out          # key -> cycle length
