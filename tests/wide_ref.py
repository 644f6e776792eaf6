"""
TEST INFRASTRUCTURE -- a plain, exact reference for networks of any size up to 1024 nodes, in numpy and Python ints.

The CPU oracle (oracle/bsx_oracle.c) holds a state in four 64-bit words and stops at 256 nodes.  This module restates
the same algorithm without a word size: a state is one uint8 per node, an index is a Python int.  It is written for
clarity, not speed, and nothing under boolsi_amd/ imports it.  tests/test_wide_ref.py proves it against the oracle
at n <= 256, field by field; tests/test_gpu_wide_exact.py then uses it above 256 nodes.

Semantics (boolsi_amd/compile.py S1 / S2 / S13, oracle/bsx_oracle.c):
  * step: next[i] = table_i[sum state[pred_i[j]] << j]; then fixed nodes; then the perturbations of the new time;
  * problem index: one binary digit per 'any' node (node order, least significant first), then one digit per
    fixed-node variation, then one per perturbation variation, radix 3 for 'any?' else 2;
  * T_p = time of the problem's last perturbation (0 without one); attractor search, target search and the recorded
    state history start at s(T_p);
  * state code = sum state[i] << i as a Python int (node n - 1 most significant).
"""
import numpy as np

DIGEST_SEED = 0xCBF29CE484222325
DIGEST_PRIME = 0x100000001B3
M64 = (1 << 64) - 1


def digit_state(range_code, digit):
    """Variation digit -> node state, None = the variation is absent (batching.py:171-175)."""
    if range_code == 0:                     # '0?'   {None, False}
        return None if digit == 0 else 0
    if range_code == 1:                     # '1?'   {None, True}
        return None if digit == 0 else 1
    if range_code == 2:                     # 'any'  {False, True}
        return digit
    return None if digit == 0 else digit - 1        # 'any?' {None, False, True}


def packed(state):
    """uint8[n] -> the state's bits as bytes, node 0 = bit 0 of byte 0."""
    return np.packbits(state, bitorder='little').tobytes()


def packed_rows(S):
    """uint8[P, n] -> list of P packed states."""
    return [r.tobytes() for r in np.packbits(S, axis=1, bitorder='little')]


def code_of(state):
    """uint8[n] (or its packed bytes) -> state code."""
    return int.from_bytes(state if isinstance(state, bytes) else packed(state), 'little')


def words_of(code, n_words):
    return [(code >> (64 * w)) & M64 for w in range(n_words)]


class Problem:
    """One decoded problem: initial state, fixed nodes (mask / value per node), perturbations {t: {node: value}}."""

    def __init__(self, init, fmask, fval, pert):
        self.init, self.fmask, self.fval, self.pert = init, fmask, fval, pert
        self.tp = max(pert) if pert else 0


class Batch:
    """A list of problems with their initial states and fixed nodes stacked, one row per problem."""

    def __init__(self, probs, n):
        self.probs = probs
        self.init = np.array([p.init for p in probs], np.uint8).reshape(len(probs), n)
        self.fmask = np.array([p.fmask for p in probs], bool).reshape(len(probs), n)
        self.fval = np.array([p.fval for p in probs], np.uint8).reshape(len(probs), n)
        self.pert_at = {}           # t -> [(problem, node, value)]
        for q, p in enumerate(probs):
            for t, entries in p.pert.items():
                self.pert_at.setdefault(t, []).extend((q, node, value) for node, value in entries.items())


class WideRef:
    def __init__(self, net, space):
        self.net, self.space = net, space
        self.n = net.n_nodes
        self.W = net.n_words
        # truth tables as one uint8 per row, unpacked from the table words (several words when k > 6)
        groups = {}
        for i in range(self.n):
            p = net.pred_idx[net.pred_offsets[i]:net.pred_offsets[i + 1]].astype(np.int64)
            words = net.tt_words[net.tt_word_offsets[i]:net.tt_word_offsets[i + 1]]
            bits = np.unpackbits(np.ascontiguousarray(words, '<u8').view(np.uint8), bitorder='little')
            g = groups.setdefault(len(p), ([], [], []))
            g[0].append(i); g[1].append(p); g[2].append(bits[:1 << len(p)])
        # number of predecessors k -> (nodes [m], predecessors [m, k], table bits [m, 2^k])
        self.by_k = {k: (np.array(nodes, np.int64), np.array(preds, np.int64).reshape(len(nodes), k), np.array(tables, np.uint8))
                     for k, (nodes, preds, tables) in groups.items()}
        self.origin = np.array([(int(space.origin_state[i >> 6]) >> (i & 63)) & 1 for i in range(self.n)], np.uint8)

    # ---- problem decoding -------------------------------------------------------------------------------------
    def problem(self, index):
        sp = self.space
        init = self.origin.copy()
        for node in sp.any_nodes.tolist():
            init[node] = index & 1
            index >>= 1
        fmask, fval = np.zeros(self.n, bool), np.zeros(self.n, np.uint8)
        for node, value in sp.fixed.tolist():
            fmask[node], fval[node] = True, value
        for node, rc in sp.fixed_var.tolist():
            radix = 3 if rc == 3 else 2
            s = digit_state(rc, index % radix)
            index //= radix
            if s is not None:
                fmask[node], fval[node] = True, s
        pert = {}
        for t, node, value in sp.sched.tolist():
            pert.setdefault(t, {})[node] = value
        for t, node, rc in sp.pert_var.tolist():
            radix = 3 if rc == 3 else 2
            s = digit_state(rc, index % radix)
            index //= radix
            if s is not None:
                pert.setdefault(t, {})[node] = s        # wins over an origin entry of the same (t, node)
        assert index == 0, 'index beyond the problem space'
        return Problem(init, fmask, fval, pert)

    # ---- one synchronous update of P problems -----------------------------------------------------------------
    def rules(self, S):
        """S uint8[P, n] -> the update rules' output, uint8[P, n].  Nodes with the same number of predecessors k are
        looked up together: row index [P, m] in S2 order, then bit `row` of each node's table."""
        N = np.empty_like(S)
        for k, (nodes, preds, tables) in self.by_k.items():
            dtype = np.uint8 if k <= 8 else np.int64        # the row index fits a byte up to k = 8
            row = np.zeros((len(S), len(nodes)), dtype)
            for j in range(k):
                row |= np.take(S, preds[:, j], axis=1).astype(dtype) << dtype(j)        # S[:, preds[:, j]]
            N[:, nodes] = tables[np.arange(len(nodes)), row]
        return N

    def advance(self, S, batch, t_next, rows=None):
        """s(t_next - 1) -> s(t_next) for the problems `rows` of the batch (default: all): rules, fixed nodes,
        then the perturbations of t_next.  S holds the states of those rows."""
        rows = np.arange(len(batch.probs)) if rows is None else np.asarray(rows, np.int64)
        N = np.where(batch.fmask[rows], batch.fval[rows], self.rules(S))
        if t_next in batch.pert_at:
            at = {q: i for i, q in enumerate(rows.tolist())}
            for q, node, value in batch.pert_at[t_next]:
                if q in at:
                    N[at[q], node] = value
        return N

    def _start(self, indices):
        batch = Batch([self.problem(int(i)) for i in indices], self.n)
        return batch, batch.init.copy()

    # ---- simulate -----------------------------------------------------------------------------------------------
    def trajectories(self, indices, t_len):
        """-> list of [t_len[q] + 1] state codes, s(0 .. t_len[q]) of problem indices[q]."""
        t_len = [int(t_len)] * len(indices) if np.isscalar(t_len) else [int(t) for t in t_len]
        batch, S = self._start(indices)
        out = [[] for _ in t_len]
        for t in range(max(t_len, default=0) + 1):
            if t:
                S = self.advance(S, batch, t)
            for q, key in enumerate(packed_rows(S)):
                if t <= t_len[q]:
                    out[q].append(code_of(key))
        return out

    def simulate(self, indices, max_t):
        """-> (trajectories as codes, final codes, digests as the oracle defines them)."""
        traj = self.trajectories(indices, max_t)
        digests = []
        for codes in traj:
            x = y = 0
            for t, c in enumerate(codes):
                x ^= c
                if (((t & 0xFFFFFFFF) * 0x9E3779B1) & 0xFFFFFFFF) >> 31:
                    y ^= c
            d = DIGEST_SEED
            for v in (x, y, codes[-1]):
                for w in words_of(v, self.W):
                    d = ((d ^ w) * DIGEST_PRIME) & M64
            digests.append(d)
        return traj, [codes[-1] for codes in traj], digests

    # ---- the search loop of attract and target (model.py:152-236 with all states stored) -----------------------
    def search(self, indices, max_t, target=None):
        """
        Every problem runs to its T_p, then until the first repeated state, a target hit or t = max_t.
        target: (nodes, values) or None.
        -> per problem a dict: tp, t (stop time), found, reached, seen ({packed state: steps since T_p});
           with found also mu and lam.
        """
        batch, S = self._start(indices)
        probs = batch.probs
        max_t = float('inf') if max_t is None else max_t
        for t in range(1, max((p.tp for p in probs), default=0) + 1):
            run = [q for q, p in enumerate(probs) if t <= p.tp]
            S[run] = self.advance(S[run], batch, t, run)

        def hits(rows):
            if target is None:
                return np.zeros(len(rows), bool)
            return (rows[:, target[0]] == target[1]).all(axis=1)

        res = [{'tp': p.tp, 't': p.tp, 'found': False, 'reached': bool(h), 'seen': {k: 0}}
               for p, h, k in zip(probs, hits(S), packed_rows(S))]
        seen = [r['seen'] for r in res]
        run = [q for q, r in enumerate(res) if r['t'] < max_t and not r['reached']]
        j = 0                               # steps since T_p: problem q is at t = T_p(q) + j
        while run:
            j += 1
            now = self.advance(S[run], batch, 0, run)           # t > T_p: no perturbation is left
            S[run] = now
            stop = set()
            for q, key in zip(run, packed_rows(now)):
                first = seen[q].setdefault(key, j)
                if first != j:                                  # s(T_p + first) again: the cycle has closed
                    res[q].update(found=True, mu=first, lam=j - first)
                    stop.add(q)
            for at in np.flatnonzero(hits(now)).tolist():
                res[run[at]]['reached'] = True
                stop.add(run[at])
            for q in run:
                res[q]['t'] = res[q]['tp'] + j
            run = [q for q in run if q not in stop and res[q]['t'] < max_t]
        return res

    def target(self, indices, max_t, nodes, code):
        """First t >= T_p with s(t)[nodes] == code[nodes]; a closed cycle or max_t ends the search.
        -> list of (reached, t_stop)."""
        nodes = np.array(sorted(nodes), np.int64)
        values = np.array([(code >> int(i)) & 1 for i in nodes], np.uint8)
        return [(r['reached'], r['t']) for r in self.search(indices, max_t, (nodes, values))]

    def attract(self, indices, max_t=None, max_len=None):
        """-> (per problem (found, key, lambda, trajectory_l = T_p + mu, t_stop), reference steps = sum of t_stop).
        found iff T_p + mu + lambda <= max_t and lambda <= max_len; a problem that is not found has key = lambda =
        trajectory_l = 0.  t_stop is the time at which the search loop ended."""
        max_len = float('inf') if max_len is None else max_len
        recs, steps = [], 0
        for r in self.search(indices, max_t):
            steps += r['t']
            if r['found'] and r['lam'] <= max_len:
                cycle = [code_of(b) for b, pos in r['seen'].items() if pos >= r['mu']]
                assert len(cycle) == r['lam']
                recs.append((True, min(cycle), r['lam'], r['tp'] + r['mu'], r['t']))
            else:
                recs.append((False, 0, 0, 0, r['t']))
        return recs, steps


def aggregate(records):
    """Per-problem attract records -> ({key: [length, count, sum_l, sum_l2]}, number without an attractor):
    the form of boolsi_amd.attract.merge_tables, in Python ints."""
    table, none = {}, 0
    for found, key, lam, tl, _ in records:
        if not found:
            none += 1
            continue
        e = table.setdefault(key, [lam, 0, 0, 0])
        assert e[0] == lam
        e[1] += 1
        e[2] += tl
        e[3] += tl * tl
    return table, none
