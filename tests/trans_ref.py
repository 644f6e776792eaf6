"""
Dict-based reference of the attractor transitions (bsx_run_attractor_transitions, include/bsx.h), for tests only.

States are Python ints (state codes).  F is the CPU oracle's `step` under the fixed mask and value of the origin problem
(Oracle.problem(0)); no perturbation schedule, no variations.  A flip x_0 is followed with every state since x_0 kept
in a dict (state -> time): the first state seen twice gives mu and lambda' by definition.  The rows of the table are
complete cycles (TransRef checks that: every row closes and no state is listed twice), so a trajectory that meets a
listed state at time t has mu = t and lambda' = that row's length, and the walk may stop there.  The same holds for the
states of an unlisted cycle that an earlier walk has closed; they are remembered with their cycle's length and key.

tests/test_trans_ref.py pins flip_outcome to the oracle's own attract, flip by flip.
"""
import numpy as np

from boolsi_amd.compile import code_to_words, words_to_code

OUTSIDE = 0xFFFFFFFE
UNRESOLVED = 0xFFFFFFFF
INF = float('inf')


class TransRef:
    def __init__(self, net, space, keys, lengths):
        from oracle.cpu_oracle import Oracle
        self.net, self.space = net, space
        self.orc = Oracle(net, space)
        rc, _, fm, fv, _ = self.orc.problem(0)
        assert rc == 0
        self.fm, self.fv = fm, fv
        fixed_mask = words_to_code(fm)
        self.free = [i for i in range(net.n_nodes) if not (fixed_mask >> i) & 1]
        self.keys, self.lengths = [int(k) for k in keys], [int(l) for l in lengths]
        self.unlisted = {}              # state of an unlisted cycle some walk has closed -> (length, key)
        self.rows = []                  # row q: its states from the key on
        self.listed = {}                # state -> row
        for q, (key, length) in enumerate(zip(self.keys, self.lengths)):
            states, s = [], key
            for _ in range(length):
                assert s not in self.listed, 'row {} shares a state with a row before it or repeats one'.format(q)
                self.listed[s] = q
                states.append(s)
                s = self.step(s)
            assert s == key, 'row {} is not closed'.format(q)
            self.rows.append(states)

    def step(self, code):
        s = code_to_words(code, self.net.n_words)
        return int(words_to_code((self.orc.step(s) & ~self.fm) | self.fv))

    def flip_outcome(self, x0, max_t=INF):
        """-> (resolved, mu, lambda', key of the cycle, row or None): the cycle x_0 ends on and whether mu + lambda' <= max_t"""
        seen, x, t = {}, x0, 0
        while True:
            d = self.listed.get(x)
            if d is not None:
                mu, lam, key = t, self.lengths[d], self.keys[d]
                break
            if x in self.unlisted:
                mu, (lam, key) = t, self.unlisted[x]
                break
            if x in seen:
                mu, lam = seen[x], t - seen[x]
                cycle = [s for s, ts in seen.items() if ts >= mu]
                key = min(cycle)
                self.unlisted.update((s, (lam, key)) for s in cycle)
                break
            seen[x] = t
            x = self.step(x)
            t += 1
        return mu + lam <= max_t, mu, lam, key, d

    def flips(self):
        """(row, index of the state in the row, node, x_0) of every flip, in the engine's order"""
        for q, states in enumerate(self.rows):
            for j, s in enumerate(states):
                for i in self.free:
                    yield q, j, i, s ^ (1 << i)

    def transitions(self, max_t=INF):
        """-> (edges, node_exits, detail): edges = sorted [(src, dst, count, sum_mu)], node_exits (n, n_nodes) uint32,
        detail = {'outside': flips onto unlisted cycles that resolve, 'unresolved': ..., 'max_mu': largest mu of a resolved flip,
                  'outside_total': flips onto unlisted cycles whether they resolve or not}"""
        acc = {}
        exits = np.zeros((len(self.rows), self.net.n_nodes), np.uint32)
        detail = {'outside': 0, 'unresolved': 0, 'max_mu': 0, 'outside_total': 0}
        listed, lengths = self.listed, self.lengths
        for q, _, i, x0 in self.flips():
            d = listed.get(x0)
            if d is not None and lengths[d] <= max_t:       # (mu = 0: the common case, kept short)
                dst, mu = d, 0
            else:
                resolved, mu, _, _, d = self.flip_outcome(x0, max_t)
                detail['outside_total'] += d is None
                if not resolved:
                    dst, mu = UNRESOLVED, 0
                    detail['unresolved'] += 1
                elif d is None:
                    dst, mu = OUTSIDE, 0
                    detail['outside'] += 1
                else:
                    dst = d
                    detail['max_mu'] = max(detail['max_mu'], mu)
            e = acc.setdefault((q, dst), [0, 0])
            e[0] += 1
            e[1] += mu
            if dst != q:
                exits[q, i] += 1
        edges = [(q, dst, c, m) for (q, dst), (c, m) in sorted(acc.items())]
        return edges, exits, detail


def cross_edges(edges):
    return [e for e in edges if e[1] != e[0] and e[1] < OUTSIDE]


def csv_rows(edges, ids, lengths, n_free):
    """the data rows of attractor_transitions.csv for `edges`; ids = first column of attractor_summaries.csv, in its order"""
    out = []
    for q, dst, count, sum_mu in edges:
        name = 'outside' if dst == OUTSIDE else 'unresolved' if dst == UNRESOLVED else ids[dst]
        mean = '' if dst >= OUTSIDE else repr(sum_mu / count)
        out.append('{},{},{},{},{}'.format(ids[q], name, count, repr(count / (lengths[q] * n_free)), mean))
    return out
