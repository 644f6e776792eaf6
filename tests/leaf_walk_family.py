"""
The network family of tests/test_gpu_leaf_walk.py (the per-parent level at a dense mirror, few parents, a full rule table);
tests/test_leaf_walk_family.py checks on the CPU that it is what it claims.

A ring of R nodes that rotate, W layer-1 nodes that fall to 0, D layer-0 nodes whose rules read 1-4 layer-1 / ring nodes
and are 0 whenever their layer-1 inputs are 0; nobody reads layer 0.  The cycle states are exactly "ring arbitrary,
everything else 0": 2^R of them, one attractor per binary necklace of the ring, mu <= 2.
"""
import random


def family_yaml(R, W, D, seed=1):
    rng = random.Random(1000 * R + 10 * W + D + seed)
    ring = ['r{}'.format(i) for i in range(R)]
    lay1 = ['a{}'.format(i) for i in range(W)]
    lay0 = ['d{}'.format(i) for i in range(D)]
    rules = {}
    for i, v in enumerate(ring):
        rules[v] = ring[(i + 1) % R]
    for v in lay1:
        rules[v] = 'r0 and not r0'
    forms = ('{a}', '{a} and {r}', '{a} and not {r}', '({a} and {r}) or {b}', '{a} and ({b} or not {r})', '{a} and ({b} or not {r}) and {c}',
             '({a} or {b}) and {r} and not {s}', '{a} and {b} and {c} and {e}', '({a} and not {b}) or ({c} and {r})')
    for j, v in enumerate(lay0):
        a = lay1[j % W]                                           # every layer-1 node is read: all W digits matter to F^1
        b, c, e = rng.sample([x for x in lay1 if x != a], 3)
        r, s = rng.sample(ring, 2)
        rules[v] = forms[(j + rng.randrange(len(forms))) % len(forms)].format(a=a, b=b, c=c, e=e, r=r, s=s)
    names = ring + lay1 + lay0
    lines = ['nodes:'] + ['    - ' + v for v in names] + ['', 'update rules:']
    lines += ['    {}: {}'.format(v, rules[v]) for v in names]
    lines += ['', 'initial state:'] + ['    {}: any'.format(v) for v in names]
    return '\n'.join(lines) + '\n'


def necklaces(ring):
    out = {}
    for v in range(1 << ring):
        orbit = {((v >> r) | (v << (ring - r))) & ((1 << ring) - 1) for r in range(ring)}
        out.setdefault(min(orbit), len(orbit))
    return out          # key -> cycle length


FAMILY = [(7, 6, 12), (6, 6, 12), (6, 10, 10), (6, 10, 33), (6, 10, 64)]
