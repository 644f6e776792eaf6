"""
TEST INFRASTRUCTURE -- reference of the attractor transitions for networks of any size up to 1024 nodes
(bsx_run_attractor_transitions_wide, include/bsx.h).  The interface of tests/trans_ref.py, on the stepping of
tests/wide_ref.py instead of the CPU oracle's: F is WideRef.rules under the fixed nodes the origin lists (no schedule,
no variations), a state is a Python int (state code).

Successors are computed in batches and remembered in a dict (state -> F(state)): all flips of a table are unpacked
into one uint8 matrix and stepped together until every trajectory has run into a state whose successor is known.
The walks themselves are then dict look-ups, as in trans_ref: a flip x_0 is followed with every state since x_0 kept
(state -> time), the first state seen twice gives mu and lambda' by definition; a listed state at time t gives mu = t
and lambda' = that row's length, because the rows are complete cycles (checked here: every row closes and no state is
listed twice).

tests/test_trans_wide_ref.py pins this module to trans_ref.TransRef at n <= 256.
"""
import numpy as np

from wide_ref import WideRef

OUTSIDE = 0xFFFFFFFE
UNRESOLVED = 0xFFFFFFFF
INF = float('inf')


class TransWideRef:
    def __init__(self, net, space, keys, lengths):
        self.net, self.space = net, space
        self.wide = WideRef(net, space)
        n = self.n = net.n_nodes
        assert len(space.fixed_var) == 0 and len(space.sched) == 0 and len(space.pert_var) == 0
        self.fmask, self.fval = np.zeros(n, bool), np.zeros(n, np.uint8)
        for node, value in space.fixed.tolist():
            self.fmask[node], self.fval[node] = True, value
        self.free = [i for i in range(n) if not self.fmask[i]]
        self.keys, self.lengths = [int(k) for k in keys], [int(l) for l in lengths]
        self.next = {}                  # state -> F(state), filled in batches
        self.unlisted = {}              # state of an unlisted cycle some walk has closed -> (length, key)
        self.rows = []                  # row q: its states from the key on
        self.listed = {}                # state -> row
        self.close(self.keys)
        for q, (key, length) in enumerate(zip(self.keys, self.lengths)):
            states, s = [], key
            for _ in range(length):
                assert s not in self.listed, 'row {} shares a state with a row before it or repeats one'.format(q)
                self.listed[s] = q
                states.append(s)
                s = self.step(s)
            assert s == key, 'row {} is not closed'.format(q)
            self.rows.append(states)

    # ---- stepping ---------------------------------------------------------------------------------------------------
    def unpack(self, codes):
        """state codes -> uint8[len(codes), n]"""
        n_bytes = (self.n + 7) // 8
        raw = np.frombuffer(b''.join(c.to_bytes(n_bytes, 'little') for c in codes), np.uint8).reshape(len(codes), n_bytes)
        return np.unpackbits(raw, axis=1, bitorder='little')[:, :self.n]

    def step_many(self, codes):
        S = self.unpack(codes)
        N = np.where(self.fmask, self.fval, self.wide.rules(S))
        return [int.from_bytes(r.tobytes(), 'little') for r in np.packbits(N, axis=1, bitorder='little')]

    def close(self, starts):
        """fills self.next along the trajectories of `starts` until each has run into a state with a known successor"""
        frontier = sorted({s for s in starts if s not in self.next})
        while frontier:
            after = self.step_many(frontier)
            self.next.update(zip(frontier, after))
            frontier = sorted({s for s in after if s not in self.next})

    def step(self, code):
        if code not in self.next:
            self.close([code])
        return self.next[code]

    # ---- the interface of trans_ref.TransRef --------------------------------------------------------------------------
    def flip_outcome(self, x0, max_t=INF):
        """-> (resolved, mu, lambda', key of the cycle, row or None): the cycle x_0 ends on and whether mu + lambda' <= max_t"""
        seen, x, t = {}, x0, 0
        while True:
            d = self.listed.get(x)
            if d is not None:
                mu, lam, key = t, self.lengths[d], min(self.rows[d])
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
        """-> (edges, node_exits, detail) as trans_ref.TransRef.transitions, and detail['mu_positive'] = resolved flips into
        a real row with mu > 0"""
        flips = list(self.flips())
        self.close([f[3] for f in flips])
        acc = {}
        exits = np.zeros((len(self.rows), self.n), np.uint32)
        detail = {'outside': 0, 'unresolved': 0, 'max_mu': 0, 'outside_total': 0, 'mu_positive': 0}
        for q, _, i, x0 in flips:
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
                detail['mu_positive'] += mu > 0
            e = acc.setdefault((q, dst), [0, 0])
            e[0] += 1
            e[1] += mu
            if dst != q:
                exits[q, i] += 1
        edges = [(q, dst, c, m) for (q, dst), (c, m) in sorted(acc.items())]
        return edges, exits, detail
