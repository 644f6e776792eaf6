"""
Python face of the gfx950 engine: one `Engine` = one bsx handle = one GPU.

The methods are thin: they marshal numpy buffers through the C-ABI (include/bsx.h) and hand back
numpy records.  All arithmetic of the hot path happens in the HIP kernels; nothing here steps a
network.  Mode drivers that mirror the reference's `*_master` functions live in attract.py /
simulate.py / target.py.
"""
import ctypes as C
from dataclasses import dataclass
from math import inf

import numpy as np

from . import _lib
from ._lib import EngineError, EngineUnavailable, Index, Stats, T_INF, ptr  # noqa: F401

_M64 = 2 ** 64 - 1


def _cap(v):
    return T_INF if v is None or v == inf else int(v)


@dataclass
class AttractResult:
    table: np.ndarray            # _lib.ATTR_REC, unordered
    n_no_attractor: int
    per_problem: np.ndarray      # _lib.PROBLEM_REC or None
    stats: dict


def key_to_int(key_words):
    v = 0
    for w, x in enumerate(np.asarray(key_words, dtype=np.uint64).tolist()):
        v |= int(x) << (64 * w)
    return v


def flat_indices(states, variants, any_nodes):
    """
    Flat problem indices I = bits + (variant << n_any) of batching.py:212-229 (what problem_from_index takes), as Python
    ints, from what bsx_sample_problems returns: states (n, W) uint64 = s(0), variants (n,) uint64; bit a of `bits` is
    the state of the a-th 'any' node, any_nodes[a], in s(0).
    """
    if len(variants) == 0:
        return []
    states = np.asarray(states, np.uint64).reshape(len(variants), -1)
    any_nodes = np.asarray(any_nodes, np.int64)
    n_any = len(any_nodes)
    if n_any == 0:
        return [int(v) for v in np.asarray(variants, np.uint64).tolist()]
    bits = (states[:, any_nodes >> 6] >> (any_nodes & 63).astype(np.uint64)) & np.uint64(1)
    packed = np.packbits(bits.astype(np.uint8), axis=1, bitorder='little')
    return [int.from_bytes(row.tobytes(), 'little') | (int(v) << n_any)
            for row, v in zip(packed, np.asarray(variants, np.uint64).tolist())]


class Engine:
    def __init__(self, device=0):
        self._lib = _lib.load()
        handle = C.c_void_p()
        rc = self._lib.bsx_create(C.byref(handle), int(device))
        if rc != 0:
            msg = self._lib.bsx_last_error(None).decode()
            raise EngineUnavailable('bsx_create(device={}) failed: {} ({})'.format(
                device, msg, self._lib.bsx_status_string(rc).decode()))
        self._h = handle
        self.device = device
        self.net = None
        self.space = None
        self._keep = []

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, '_h', None):
            self._lib.bsx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001  (interpreter shutdown)
            pass

    def _check(self, rc):
        if rc != 0:
            raise EngineError(rc, self._lib.bsx_last_error(self._h).decode() or
                              self._lib.bsx_status_string(rc).decode())

    def device_info(self):
        name = C.create_string_buffer(256)
        cus = C.c_uint32()
        mem = C.c_uint64()
        self._check(self._lib.bsx_device_info(self._h, name, 256, C.byref(cus), C.byref(mem)))
        return {'name': name.value.decode(), 'compute_units': cus.value, 'global_mem_bytes': mem.value}

    def network_info(self):
        """How the network was lowered: names the kernel instantiations a run launches (bsx_network_info)."""
        nw, k, lm = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(self._lib.bsx_network_info(self._h, C.byref(nw), C.byref(k), C.byref(lm)))
        return {'state_words32': nw.value, 'mux_slots': k.value, 'lut_mode': lm.value}

    def synchronize(self):
        self._check(self._lib.bsx_synchronize(self._h))

    # -- multi-GPU merge step (RCCL through the C-ABI; driven by boolsi_amd.dist.Comm) -----------
    def comm_unique_id(self):
        buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
        self._check(self._lib.bsx_comm_unique_id(self._h, buf, _lib.COMM_ID_BYTES))
        return buf.raw

    def comm_init(self, unique_id, rank, world):
        self._check(self._lib.bsx_comm_init(self._h, unique_id, len(unique_id), int(rank), int(world)))

    def comm_allgather(self, send, world):
        """send: contiguous uint8 array, same size on every rank -> uint8 array of world * size bytes."""
        send = np.ascontiguousarray(send, np.uint8)
        recv = np.zeros(world * send.size, np.uint8)
        self._check(self._lib.bsx_comm_allgather(self._h, ptr(send), send.size, ptr(recv)))
        return recv

    def comm_destroy(self):
        if getattr(self, '_h', None):
            self._check(self._lib.bsx_comm_destroy(self._h))

    # -- problem definition -----------------------------------------------------------------
    def set_problem(self, net, space):
        """net, space: boolsi_amd.compile.CompiledNetwork / CompiledSpace."""
        a = [np.ascontiguousarray(x) for x in (net.pred_offsets, net.pred_idx, net.tt_word_offsets,
                                               net.tt_words)]
        self._check(self._lib.bsx_set_network(self._h, net.n_nodes, ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3])))
        self.net = net
        self._keep_net = a
        self.set_space(space)

    def set_space(self, space):
        b = [np.ascontiguousarray(space.origin_state, np.uint64),
             np.ascontiguousarray(space.any_nodes, np.uint32),
             np.ascontiguousarray(space.fixed, np.uint32), np.ascontiguousarray(space.fixed_var, np.uint32),
             np.ascontiguousarray(space.sched, np.uint32), np.ascontiguousarray(space.pert_var, np.uint32)]
        self._check(self._lib.bsx_set_problem_space(
            self._h, ptr(b[0]), ptr(b[1]), len(b[1]), ptr(b[2]), len(b[2]), ptr(b[3]), len(b[3]),
            ptr(b[4]), len(b[4]), ptr(b[5]), len(b[5])))
        self.space = space
        self._keep = b

    def states_from(self, state_code, n_steps):
        """
        s, f(s), ..., f^n_steps(s) for the state with code `state_code`, under the origin problem's
        constant fixed nodes and without perturbations -> (n_steps + 1, W) uint64 array.
        Used to list the states of an attractor from its key (reference attract.py:22-25 keeps
        them in memory instead).
        """
        from .compile import CompiledSpace, code_to_words
        saved = self.space
        empty2 = np.zeros((0, 2), np.uint32)
        empty3 = np.zeros((0, 3), np.uint32)
        tmp = CompiledSpace(n_nodes=self.net.n_nodes, origin_state=code_to_words(state_code, self.net.n_words),
                            any_nodes=np.zeros(0, np.uint32), fixed=saved.fixed, fixed_var=empty2, sched=empty3,
                            pert_var=empty3, n_problems=1, radices=[])
        self.set_space(tmp)
        try:
            trajs, _ = self.trajectories(0, [0], [n_steps])
        finally:
            self.set_space(saved)
        return trajs[0]

    def attractor_profile(self, keys, lengths, states=True, activity=True):
        """
        The attractors (key state code, length) of a whole table in one device call (bsx_run_attractor_profile):
        every cycle is walked from its key under the origin problem's fixed nodes, without perturbations.
        -> (on_counts, states, closed):
           on_counts  (n, n_nodes) uint32, in how many of the cycle's states each node is on; None without `activity`
           states     list of (length, W) uint64 arrays, first state = the key; None without `states`
           closed     uint8 array, 1 iff f^length(key) == key
        The problem space and the cycle-state cache of the engine are left as they are; `profile_stats` holds the
        call's statistics afterwards.
        """
        W = self.net.n_words
        n = len(keys)
        ints = [int(k) for k in keys]               # Python ints: what merge_tables produces
        if any(k < 0 or k >> (64 * W) for k in ints):
            raise ValueError('a key does not fit the {} words of a state'.format(W))
        key_words = np.zeros((n, W), np.uint64)
        for w in range(W):
            key_words[:, w] = [(k >> (64 * w)) & _M64 for k in ints]
        lens = np.ascontiguousarray(lengths, np.uint64)
        if lens.shape != (n,):
            raise ValueError('one length per key')
        on_counts = np.zeros((n, self.net.n_nodes), np.uint32) if activity else None
        closed = np.zeros(n, np.uint8)
        out = offsets = None
        if states:
            sizes = lens * np.uint64(W)
            offsets = np.zeros(n, np.uint64)
            if n > 1:
                offsets[1:] = np.cumsum(sizes[:-1])
            out = np.zeros(int(sizes.sum()), np.uint64)
        st = Stats()
        self._run_attractor_profile(ptr(key_words), W, ptr(lens), n, ptr(on_counts), ptr(out), ptr(offsets), ptr(closed), st)
        self.profile_stats = st.as_dict()
        listed = None
        if states:
            listed = [out[int(o):int(o) + int(l) * W].reshape(-1, W) for o, l in zip(offsets, lens)]
        return on_counts, listed, closed

    def _run_attractor_profile(self, keys, key_stride, lengths, n, on_counts, states, state_offsets, closed, stats):
        """The ABI call itself; null pointers for the outputs that were not asked for."""
        self._check(self._lib.bsx_run_attractor_profile(self._h, keys, key_stride, lengths, n, on_counts, states,
                                                        state_offsets, closed, C.byref(stats)))

    def node_correlations(self, keys, lengths, frequencies, ranks=False, activity=False):
        """
        The matrix behind the frequency-weighted Spearman correlations of a whole attractor table in one device call
        (bsx_run_node_correlations): attractor q = (key state code, length), occurring frequencies[q] times.
        -> (S, ranks, on_counts, closed):
           S          (n_nodes, n_nodes) float64, S[a][b] = sum_q f_q d2[q][a] d2[q][b] with d2 twice the centred average
                      rank; rho = S[a][b] / sqrt(S[a][a] S[b][b]); symmetric and reproducible bit for bit
           ranks      (n, n_nodes) float64 average weighted ranks; None without `ranks`
           on_counts  (n, n_nodes) uint32 as attractor_profile; None without `activity`
           closed     uint8 array, 1 iff f^length(key) == key
        An EngineError with status ERR_RANGE_TOO_LARGE (total frequency of 2^62 or more) or ERR_UNSUPPORTED (more than
        2^31 cells) means the table is for the host path.  `corr_stats` holds the call's statistics afterwards.
        """
        W, n_nodes = self.net.n_words, self.net.n_nodes
        n = len(keys)
        ints = [int(k) for k in keys]
        if any(k < 0 or k >> (64 * W) for k in ints):
            raise ValueError('a key does not fit the {} words of a state'.format(W))
        key_words = np.zeros((n, W), np.uint64)
        for w in range(W):
            key_words[:, w] = [(k >> (64 * w)) & _M64 for k in ints]
        lens = np.ascontiguousarray(lengths, np.uint64)
        freqs = [int(f) for f in frequencies]
        if lens.shape != (n,) or len(freqs) != n:
            raise ValueError('one length and one frequency per key')
        if any(f < 0 or f >> 128 for f in freqs):
            raise ValueError('a frequency does not fit 128 bits')
        freq_words = np.zeros((n, 2), np.uint64)
        freq_words[:, 0] = [f & _M64 for f in freqs]
        freq_words[:, 1] = [f >> 64 for f in freqs]
        s_matrix = np.zeros((n_nodes, n_nodes), np.float64)
        rank_out = np.zeros((n, n_nodes), np.float64) if ranks else None
        on_counts = np.zeros((n, n_nodes), np.uint32) if activity else None
        closed = np.zeros(n, np.uint8)
        st = Stats()
        self._run_node_correlations(ptr(key_words), W, ptr(lens), ptr(freq_words), n, ptr(s_matrix), ptr(rank_out),
                                    ptr(on_counts), ptr(closed), st)
        self.corr_stats = st.as_dict()
        return s_matrix, rank_out, on_counts, closed

    def _run_node_correlations(self, keys, key_stride, lengths, frequencies, n, s_matrix, ranks, on_counts, closed, stats):
        """The ABI call itself; null pointers for the outputs that were not asked for."""
        self._check(self._lib.bsx_run_node_correlations(self._h, keys, key_stride, lengths, frequencies, n, s_matrix, ranks,
                                                        on_counts, closed, C.byref(stats)))

    def attractor_transitions(self, keys, lengths, max_t=float('inf'), edge_cap=1 << 20, node_exits=False):
        """
        Where every single-node flip of every cycle state of the listed attractors ends, in one device call
        (bsx_run_attractor_transitions): attractor q = (key state code, length), walked under the origin problem's fixed
        nodes without perturbations; one flip per (attractor, cycle state, node that the origin does not fix).
        -> (edges, node_exits, closed):
           edges       TRANS_EDGE records (src, dst, count, sum_mu) sorted by (src, dst); dst is a row of the table,
                       _lib.TRANS_OUTSIDE (a cycle in no row) or _lib.TRANS_UNRESOLVED (mu + lambda > max_t); sum_mu is the
                       sum of the recovery times of the `count` flips (0 for the two pseudo-destinations)
           node_exits  (n, n_nodes) uint32, how many flips of node i from attractor q did not return to q; None unless asked
           closed      uint8 array, 1 iff f^length(key) == key
        An EngineError with status ERR_INVALID names a row that is not closed or shares a state with another row,
        ERR_TABLE_FULL means more distinct edges than `edge_cap`, ERR_UNSUPPORTED a network on the wide-state family.
        `trans_stats` holds the call's statistics afterwards.
        """
        return self._attractor_transitions(self._lib.bsx_run_attractor_transitions, keys, lengths, max_t, edge_cap, node_exits)

    def attractor_transitions_wide(self, keys, lengths, max_t=float('inf'), edge_cap=1 << 20, node_exits=False):
        """
        attractor_transitions for networks of every supported size (bsx_run_attractor_transitions_wide): the same
        arguments and the same (edges, node_exits, closed).  On the wide-state family a row may be listed from any state
        of its cycle, and ERR_INVALID names a row that is not closed or lies on the cycle of another row; below 257 nodes
        (without BSX_WIDE=1) the call is attractor_transitions.
        """
        return self._attractor_transitions(self._lib.bsx_run_attractor_transitions_wide, keys, lengths, max_t, edge_cap, node_exits)

    def _attractor_transitions(self, call, keys, lengths, max_t, edge_cap, node_exits):
        W = self.net.n_words
        n = len(keys)
        ints = [int(k) for k in keys]
        if any(k < 0 or k >> (64 * W) for k in ints):
            raise ValueError('a key does not fit the {} words of a state'.format(W))
        key_words = np.zeros((n, W), np.uint64)
        for w in range(W):
            key_words[:, w] = [(k >> (64 * w)) & _M64 for k in ints]
        lens = np.ascontiguousarray(lengths, np.uint64)
        if lens.shape != (n,):
            raise ValueError('one length per key')
        cap = _lib.T_INF if max_t is None or max_t == float('inf') else int(max_t)
        edges = np.zeros(int(edge_cap), _lib.TRANS_EDGE)
        exits = np.zeros((n, self.net.n_nodes), np.uint32) if node_exits else None
        closed = np.zeros(n, np.uint8)
        n_edges = C.c_uint64(0)
        st = Stats()
        self._check(call(self._h, ptr(key_words), W, ptr(lens), n, cap, edges.ctypes.data_as(C.c_void_p), int(edge_cap),
                         C.byref(n_edges), ptr(exits), ptr(closed), C.byref(st)))
        self.trans_stats = st.as_dict()
        return edges[:n_edges.value].copy(), exits, closed

    def index(self, i):
        """python int problem index -> bsx_index (split at the initial-state digits)."""
        n_any = len(self.space.any_nodes)
        low = i & ((1 << n_any) - 1)
        ix = Index()
        for w in range(_lib.MAX_WORDS):
            ix.init_digits[w] = (low >> (64 * w)) & _M64
        variant = i >> n_any
        if variant > _M64:
            raise ValueError('variant part of the problem index exceeds 64 bits')
        ix.variant = variant
        return ix

    # -- runs ---------------------------------------------------------------------------------
    def attract_fgraph(self, first, count, max_t=inf, max_len=inf, cap=65536):
        """attract through the functional graph (spaces with n <= 32 nodes, all 'any'); same result as attract."""
        table = np.zeros(cap, _lib.ATTR_REC)
        n_out, none, st = C.c_uint32(), C.c_uint64(), Stats()
        self._check(self._lib.bsx_run_attract_fgraph(self._h, C.byref(self.index(first)), count, _cap(max_t), _cap(max_len),
                                                     ptr(table), cap, C.byref(n_out), C.byref(none), C.byref(st)))
        return AttractResult(table[:n_out.value].copy(), none.value, None, st.as_dict())

    def attract(self, first, count, max_t=inf, max_len=inf, per_problem=False, cap=65536):
        # the output table is reused between calls (the library fills table[0..n_out), which is copied out)
        table = getattr(self, '_attr_table', None)
        if table is None or len(table) < cap:
            table = self._attr_table = np.zeros(cap, _lib.ATTR_REC)
        pp = np.zeros(count, _lib.PROBLEM_REC) if per_problem else None
        n_out = C.c_uint32()
        none = C.c_uint64()
        st = Stats()
        rc = self._lib.bsx_run_attract(self._h, C.byref(self.index(first)), count, _cap(max_t), _cap(max_len),
                                       ptr(table), cap, C.byref(n_out), C.byref(none), ptr(pp) if per_problem else None,
                                       C.byref(st))
        self._check(rc)
        return AttractResult(table[:n_out.value].copy(), none.value, pp, st.as_dict())

    def attract2(self, first, count, max_t=inf, max_len=inf, cap=65536):
        """attract over [first, first + count) for flat problem indices / counts of up to 128 bits (bsx_run_attract2):
        one call for the whole range however large -> AttractResult with a _lib.ATTR_REC2 table (wide sums)."""
        table = getattr(self, '_attr_table2', None)
        if table is None or len(table) < cap:
            table = self._attr_table2 = np.zeros(cap, _lib.ATTR_REC2)
        n_out, none, st = C.c_uint32(), _lib.U128(), _lib.Stats2()
        self._check(self._lib.bsx_run_attract2(self._h, _lib.U128.of(first), _lib.U128.of(count), _cap(max_t), _cap(max_len),
                                               ptr(table), cap, C.byref(n_out), C.byref(none), C.byref(st)))
        return AttractResult(table[:n_out.value].copy(), int(none), None, st.as_dict())

    @property
    def wide(self):
        """The current network runs on the wide-state family (more than 256 nodes, or BSX_WIDE=1)."""
        return self.network_info()['lut_mode'] == _lib.LUT_WIDE

    def attract_wide(self, first, count, max_t=inf, max_len=inf, cap=65536):
        """bsx_run_attract_wide: attract2 for networks of any supported size -> table of _lib.ATTR_REC2W."""
        table = getattr(self, '_attr_table2w', None)
        if table is None or len(table) < cap:
            table = self._attr_table2w = np.zeros(cap, _lib.ATTR_REC2W)
        n_out, none, st = C.c_uint32(), _lib.U128(), _lib.Stats2()
        self._check(self._lib.bsx_run_attract_wide(self._h, _lib.U128.of(first), _lib.U128.of(count), _cap(max_t),
                                                   _cap(max_len), ptr(table), cap, C.byref(n_out), C.byref(none),
                                                   C.byref(st)))
        return AttractResult(table[:n_out.value].copy(), int(none), None, st.as_dict())

    def attract_sampled(self, seed, first, count, max_t=inf, max_len=inf, cap=65536):
        """bsx_run_attract_sampled: attract over samples [first, first + count) of `seed` (include/bsx.h defines sample
        j) -> AttractResult with a _lib.ATTR_REC2W table; count of a record = samples that reached it."""
        table = getattr(self, '_attr_table2w', None)
        if table is None or len(table) < cap:
            table = self._attr_table2w = np.zeros(cap, _lib.ATTR_REC2W)
        n_out, none, st = C.c_uint32(), C.c_uint64(), _lib.Stats2()
        self._check(self._lib.bsx_run_attract_sampled(self._h, int(seed), int(first), int(count), _cap(max_t), _cap(max_len),
                                                      ptr(table), cap, C.byref(n_out), C.byref(none), C.byref(st)))
        return AttractResult(table[:n_out.value].copy(), none.value, None, st.as_dict())

    def sample_problems(self, seed, samples):
        """bsx_sample_problems: the problems behind the listed sample numbers of `seed`
        -> (states (n, W) uint64: s(0) of each sample, variants (n,) uint64: its variant number)."""
        samples = np.ascontiguousarray(samples, np.uint64)
        states = np.zeros((len(samples), self.net.n_words), np.uint64)
        variants = np.zeros(len(samples), np.uint64)
        self._check(self._lib.bsx_sample_problems(self._h, int(seed), ptr(samples), len(samples), ptr(states), ptr(variants)))
        return states, variants

    def sample_flat_indices(self, seed, samples):
        """Flat problem indices of the listed samples of `seed` (flat_indices over sample_problems), as Python ints."""
        states, variants = self.sample_problems(seed, samples)
        return flat_indices(states, variants, self.space.any_nodes)

    def target_sampled(self, seed, first, count, max_t, mask_words, code_words, hist_bins=0, cap=0):
        """bsx_run_target_sampled: target_summary over samples [first, first + count) of `seed`
        -> (n_hits, histogram of first-hit times (last bin = that time or later), the first min(n_hits, cap) hits in
        sample order with offset = sample - first, stats)."""
        hist = np.zeros(max(hist_bins, 1), np.uint64)
        hits = np.zeros(max(cap, 1), _lib.HIT)
        m = np.ascontiguousarray(mask_words, np.uint64)
        c = np.ascontiguousarray(code_words, np.uint64)
        n_hits, n_listed = C.c_uint64(), C.c_uint64()
        st = Stats()
        self._check(self._lib.bsx_run_target_sampled(
            self._h, int(seed), int(first), int(count), _cap(max_t), ptr(m), ptr(c), ptr(hist) if hist_bins else None,
            hist_bins, ptr(hits) if cap else None, cap, C.byref(n_hits), C.byref(n_listed), C.byref(st)))
        return n_hits.value, hist[:hist_bins], hits[:n_listed.value], st.as_dict()

    def simulate_sampled(self, seed, first, count, max_t, trajectories=True, final=True, digest=True):
        """bsx_run_simulate_sampled: simulate over samples [first, first + count) of `seed`."""
        W = self.net.n_words
        traj = np.zeros((count, max_t + 1, W), np.uint64) if trajectories else None
        fin = np.zeros((count, W), np.uint64) if final else None
        dig = np.zeros(count, np.uint64) if digest else None
        st = Stats()
        self._check(self._lib.bsx_run_simulate_sampled(self._h, int(seed), int(first), int(count), int(max_t),
                                                       ptr(traj) if trajectories else None, ptr(fin) if final else None,
                                                       ptr(dig) if digest else None, C.byref(st)))
        return traj, fin, dig, st.as_dict()

    def damage_sampled(self, seed, first, count, n_flips, n_steps, hist=False):
        """bsx_run_damage_sampled: damage spreading over samples [first, first + count) of `seed` (include/bsx.h has the
        definition) -> (sum_d, sum_d2, n_merged: uint64 (n_steps + 1,); hist: uint64 (n_steps + 1, n + 1) or None; stats)."""
        n_t = int(n_steps) + 1
        sum_d, sum_d2, merged = (np.zeros(n_t, np.uint64) for _ in range(3))
        cells = np.zeros((n_t, self.net.n_nodes + 1), np.uint64) if hist else None
        st = Stats()
        self._check(self._lib.bsx_run_damage_sampled(self._h, int(seed), int(first), int(count), int(n_flips), int(n_steps),
                                                     ptr(sum_d), ptr(sum_d2), ptr(merged), ptr(cells) if hist else None,
                                                     C.byref(st)))
        return sum_d, sum_d2, merged, cells, st.as_dict()

    def screen_sampled(self, seed, first, count, mutants, max_t=inf, max_len=inf, cap=None):
        """bsx_run_screen_sampled: a knockout / overexpression screen over samples [first, first + count) of `seed`
        (include/bsx.h has the definition).  mutants: a list of mutants, each a sequence of (node, value) pairs, the empty
        one the wild type -> (records per mutant: a list of _lib.ATTR_REC2W arrays in key order, samples without an
        attractor per mutant: uint64 (len(mutants),), stats)."""
        mutants = [list(m) for m in mutants]
        offsets = np.zeros(len(mutants) + 1, np.uint32)
        offsets[1:] = np.cumsum([len(m) for m in mutants])
        nodes = np.zeros(max(int(offsets[-1]), 1), _lib.FIXED)
        for i, (node, value) in enumerate(pair for m in mutants for pair in m):
            nodes[i] = (int(node), int(value))
        if cap is None:         # at most one record per trajectory, and never more than the device reduces
            cap = max(1, min(len(mutants) * int(count), 1 << 20))
        table = np.zeros(max(int(cap), 1), _lib.SCREEN_REC)
        none = np.zeros(max(len(mutants), 1), np.uint64)
        n_out, st = C.c_uint64(), _lib.Stats2()
        self._check(self._lib.bsx_run_screen_sampled(self._h, int(seed), int(first), int(count), ptr(offsets), ptr(nodes), len(mutants),
                                                     _cap(max_t), _cap(max_len), ptr(table), int(cap), C.byref(n_out), ptr(none),
                                                     C.byref(st)))
        got = table[:n_out.value]
        cuts = np.searchsorted(got['mutant'], np.arange(len(mutants) + 1, dtype=np.uint64))
        return [got['rec'][cuts[m]:cuts[m + 1]].copy() for m in range(len(mutants))], none[:len(mutants)], st.as_dict()

    def influence_sampled(self, seed, first, count, sources, n_steps, merged=True):
        """bsx_run_influence_sampled: the influence matrix over samples [first, first + count) of `seed` (include/bsx.h has
        the definition).  sources: distinct nodes the origin does not fix, in any order -> (influence: uint32 (n_sources,
        n_steps, n), the samples in which the target differs at t = 1 .. n_steps after the source was inverted at t = 0;
        n_merged: uint64 (n_sources, n_steps) or None; stats)."""
        src = np.ascontiguousarray(sources, np.uint32)
        n_steps = int(n_steps)
        table = np.zeros((len(src), n_steps, self.net.n_nodes), np.uint32)
        gone = np.zeros((len(src), n_steps), np.uint64) if merged else None
        st = Stats()
        self._check(self._lib.bsx_run_influence_sampled(self._h, int(seed), int(first), int(count), ptr(src), len(src), n_steps,
                                                        ptr(table), ptr(gone) if merged else None, C.byref(st)))
        return table, gone, st.as_dict()

    def trajectories_sampled(self, seed, samples, t_len):
        """States s(0..t_len[q]) of samples samples[q] of `seed` -> list of (t_len[q] + 1, W) arrays."""
        W = self.net.n_words
        samples = np.ascontiguousarray(samples, np.uint64)
        t_len = np.ascontiguousarray(t_len, np.uint64)
        sizes = (t_len + np.uint64(1)) * np.uint64(W)
        out_off = np.zeros(len(samples), np.uint64)
        if len(samples) > 1:
            out_off[1:] = np.cumsum(sizes[:-1])
        out = np.zeros(int(sizes.sum()), np.uint64)
        st = Stats()
        self._check(self._lib.bsx_run_trajectories_sampled(self._h, int(seed), ptr(samples), ptr(t_len), len(samples),
                                                           ptr(out), ptr(out_off), C.byref(st)))
        return [out[int(o):int(o) + int(s)].reshape(-1, W) for o, s in zip(out_off, sizes)], st.as_dict()

    def target(self, first, count, max_t, mask_words, code_words, cap=None):
        cap = count if cap is None else cap
        hits = np.zeros(max(cap, 1), _lib.HIT)
        m = np.ascontiguousarray(mask_words, np.uint64)
        c = np.ascontiguousarray(code_words, np.uint64)
        n_hits = C.c_uint64()
        st = Stats()
        self._check(self._lib.bsx_run_target(self._h, C.byref(self.index(first)), count, _cap(max_t), ptr(m), ptr(c),
                                             ptr(hits), cap, C.byref(n_hits), C.byref(st)))
        return hits[:n_hits.value], st.as_dict()      # ascending offset order (ABI contract)

    def target_summary(self, first, count, max_t, mask_words, code_words, hist_bins=0, cap=0):
        """Hits counted on the device: -> (n_hits, histogram of first-hit times (last bin = that time or later),
        the first min(n_hits, cap) hits in index order, stats).  Nothing per problem crosses PCIe."""
        hist = np.zeros(max(hist_bins, 1), np.uint64)
        hits = np.zeros(max(cap, 1), _lib.HIT)
        m = np.ascontiguousarray(mask_words, np.uint64)
        c = np.ascontiguousarray(code_words, np.uint64)
        n_hits, n_listed = C.c_uint64(), C.c_uint64()
        st = Stats()
        self._check(self._lib.bsx_run_target_summary(
            self._h, C.byref(self.index(first)), count, _cap(max_t), ptr(m), ptr(c), ptr(hist) if hist_bins else None,
            hist_bins, ptr(hits) if cap else None, cap, C.byref(n_hits), C.byref(n_listed), C.byref(st)))
        return n_hits.value, hist[:hist_bins], hits[:n_listed.value], st.as_dict()

    def simulate(self, first, count, max_t, trajectories=True, final=True, digest=True):
        W = self.net.n_words
        traj = np.zeros((count, max_t + 1, W), np.uint64) if trajectories else None
        fin = np.zeros((count, W), np.uint64) if final else None
        dig = np.zeros(count, np.uint64) if digest else None
        st = Stats()
        self._check(self._lib.bsx_run_simulate(self._h, C.byref(self.index(first)), count, int(max_t),
                                               ptr(traj) if trajectories else None, ptr(fin) if final else None,
                                               ptr(dig) if digest else None, C.byref(st)))
        return traj, fin, dig, st.as_dict()

    def trajectories(self, first, offsets, t_len):
        """States s(0..t_len[q]) of problems first + offsets[q] -> list of (t_len[q] + 1, W) arrays."""
        W = self.net.n_words
        offsets = np.ascontiguousarray(offsets, np.uint64)
        t_len = np.ascontiguousarray(t_len, np.uint64)
        sizes = (t_len + np.uint64(1)) * np.uint64(W)
        out_off = np.zeros(len(offsets), np.uint64)
        if len(offsets) > 1:
            out_off[1:] = np.cumsum(sizes[:-1])
        out = np.zeros(int(sizes.sum()), np.uint64)
        st = Stats()
        self._check(self._lib.bsx_run_trajectories(self._h, C.byref(self.index(first)), ptr(offsets), ptr(t_len),
                                                   len(offsets), ptr(out), ptr(out_off), C.byref(st)))
        return [out[int(o):int(o) + int(s)].reshape(-1, W) for o, s in zip(out_off, sizes)], st.as_dict()
