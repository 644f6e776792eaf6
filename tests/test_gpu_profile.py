"""
bsx_run_attractor_profile / Engine.attractor_profile: states, per-node on-counts and closure of a whole attractor
table in one device call.  Every comparison is exact equality.

References: up to 256 nodes the CPU oracle's `step` with the origin problem's fixed mask and value applied
(Oracle.problem(0)); above, the stepping of tests/wide_ref.py; and for both families the engine's own states_from,
one attractor at a time.  Each case asserts from the reference alone that it is not vacuous before it looks at the
engine.  The seeds were chosen on the CPU so that those guards hold.

The cases for networks of up to 256 nodes are plain functions of an engine: the tests call them, and
test_narrow_cases_on_the_wide_family runs them once more in a fresh child process with BSX_WIDE=1, where the same
networks are lowered to the wide-state family.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == '__main__':
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from boolsi_amd import synth
from boolsi_amd.attract import AggregatedAttractor, attract_master, run_attract_range
from boolsi_amd.attractor_analysis import find_node_correlations
from boolsi_amd.compile import code_to_words, compile_problem, words_to_code
from boolsi_amd.constants import Mode
from boolsi_amd.engine import Engine, EngineError
from boolsi_amd.input import parse_input_text
from boolsi_amd.model import decode_state

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_STEP_LIMIT, ERR_STATE = -1, -6, -7


# ---- networks (pure functions of their arguments) ---------------------------------------------------------------------

def yaml_of(preds, masks, init, fixed=None):
    n = len(preds)
    out = ['nodes:'] + ['    - {}'.format(synth.node_name(i)) for i in range(n)] + ['', 'update rules:']
    out += ['    {}: {}'.format(synth.node_name(i), synth.rule_text(preds[i], masks[i])) for i in range(n)]
    out += ['', 'initial state:'] + ['    {}: {}'.format(synth.node_name(i), init[i]) for i in range(n)]
    if fixed:
        out += ['', 'fixed nodes:'] + ["    {}: '{}'".format(synth.node_name(i), s) for i, s in fixed.items()]
    return '\n'.join(out) + '\n'


@functools.lru_cache(maxsize=None)
def compiled(text):
    cfg = parse_input_text(text, float('inf'), Mode.ATTRACT)
    net, space = compile_problem(cfg)
    return cfg, net, space


def add_lfsr(preds, masks, nodes, tap):
    """Fibonacci LFSR over `nodes` (in register order): nodes[0] <- nodes[-1] XOR nodes[tap - 1], nodes[i] <- nodes[i - 1]."""
    a, b = sorted((nodes[-1], nodes[tap - 1]))
    preds[nodes[0]], masks[nodes[0]] = [a, b], 0b0110
    for i in range(1, len(nodes)):
        preds[nodes[i]], masks[nodes[i]] = [nodes[i - 1]], 0b10


def add_identity(preds, masks, nodes):
    for i in nodes:
        preds[i], masks[i] = [i], 0b10


def block_network(n, identity, lfsr, tap):
    """n nodes: an identity block, an LFSR block, every other node constant 0; the block nodes are 'any'."""
    preds, masks, init = [[] for _ in range(n)], [0] * n, ['0'] * n
    add_identity(preds, masks, identity)
    add_lfsr(preds, masks, lfsr, tap)
    for i in list(identity) + list(lfsr):
        init[i] = 'any'
    return yaml_of(preds, masks, init)


def lfsr_text(n, tap):
    return block_network(n, [], list(range(n)), tap)


MIXED = block_network(16, list(range(6)), list(range(6, 16)), 7)       # 6 identity nodes + the 10-node LFSR: 128 attractors


def random_text(n, seed, n_any=10, fixed=None, many_preds=False):
    preds, masks = synth.random_network(n, 2, seed)
    if many_preds:          # one node with 9 predecessors (beyond the 6 of the mux tree)
        import random
        rng = random.Random(seed + 5)
        preds[n // 2], masks[n // 2] = sorted(rng.sample(range(n), 9)), rng.getrandbits(512)
    bits = synth.seeded_bits(n, seed + 3)
    init = ['any' if i < n_any else str(bits[i]) for i in range(n)]
    return yaml_of(preds, masks, init, fixed)


# ---- references ---------------------------------------------------------------------------------------------------------

def oracle_of(net, space):
    from oracle.cpu_oracle import Oracle
    return Oracle(net, space)


def oracle_walk(net, space, key, length):
    """-> ((length, W) states from the key, f^length(key)) by the oracle's step under the origin's fixed nodes"""
    orc = oracle_of(net, space)
    rc, _, fm, fv, _ = orc.problem(0)
    assert rc == 0
    s = code_to_words(key, net.n_words)
    out = np.zeros((length, net.n_words), np.uint64)
    for t in range(length):
        out[t] = s
        s = (orc.step(s) & ~fm) | fv
    return out, s


def counts_of(states, n):
    """per-node on-counts of (length, W) packed states, by plain integer counting"""
    bits = np.unpackbits(np.ascontiguousarray(states, '<u8').view(np.uint8).reshape(len(states), -1), axis=1, bitorder='little')
    return bits[:, :n].sum(axis=0, dtype=np.uint64).astype(np.uint32)


def oracle_table(net, space, count):
    """{key: length} of the attractors the oracle finds from problems [0, count)"""
    from oracle.cpu_oracle import key_int
    _, table, none, _ = oracle_of(net, space).attract(0, count)
    assert none == 0
    return {key_int(r['key']): int(r['length']) for r in table}


def check_against_references(eng, net, space, keys, lengths, with_states_from=True):
    """one call for all attractors; on-counts, states, closed against the oracle walk and (optionally) states_from"""
    on, states, closed = eng.attractor_profile(keys, lengths)
    assert on.shape == (len(keys), net.n_nodes) and on.dtype == np.uint32 and len(states) == len(keys)
    # one launch per BSX_PROFILE_CHUNK attractors, on the wide family per BSX_PROFILE_CHUNK_WIDE (include/bsx.h)
    assert eng.profile_stats['kernel_launches'] == -(-len(keys) // (1 << 18 if eng.wide else 1 << 22)) == 1
    for q, (key, length) in enumerate(zip(keys, lengths)):
        want, back = oracle_walk(net, space, key, length)
        assert words_to_code(back) == key, 'reference: the key is not on a cycle of this length'
        assert np.array_equal(states[q], want), (q, key)
        assert np.array_equal(on[q], counts_of(want, net.n_nodes)), (q, key)
        assert closed[q] == 1
        if with_states_from:
            assert np.array_equal(eng.states_from(key, length - 1), want), (q, key)
    # the same attractors without states: no state crosses, the counts are the same
    on2, none, closed2 = eng.attractor_profile(keys, lengths, states=False)
    assert none is None and np.array_equal(on2, on) and np.array_equal(closed2, closed)
    on3, states3, _ = eng.attractor_profile(keys, lengths, activity=False)
    assert on3 is None and all(np.array_equal(a, b) for a, b in zip(states3, states))


# ---- cases for networks of up to 256 nodes (also run under BSX_WIDE=1, see the module docstring) ------------------------

def lfsr_cycle_length(n, tap):
    """plain Python: steps until the register returns to 1"""
    s, t = 1, 0
    while True:
        bit = ((s >> (n - 1)) ^ (s >> (tap - 1))) & 1
        s = ((s << 1) | bit) & ((1 << n) - 1)
        t += 1
        if s == 1:
            return t


def case_long_cycle(eng, n, tap):
    """Fibonacci LFSR: lambda = 2^n - 1 from every non-zero state, every node on in 2^(n-1) of them"""
    lam = (1 << n) - 1
    assert lfsr_cycle_length(n, tap) == lam                               # guard: maximal length
    _, net, space = compiled(lfsr_text(n, tap))
    # every node is 'any' and nothing is fixed or perturbed: problem 1 starts at state 1, the smallest non-zero code and so
    # the cycle's key, and the oracle's trajectory is its step applied lam times (checked against step itself at the start)
    traj = oracle_of(net, space).trajectory(1, lam)
    want, back = traj[:lam], traj[lam]
    assert np.array_equal(oracle_walk(net, space, 1, 300)[0], want[:300])
    assert words_to_code(back) == 1 and len({int(w) for w in want[:, 0]}) == lam
    eng.set_problem(net, space)
    on, states, closed = eng.attractor_profile([1, 0], [lam, 1])
    assert on[0].tolist() == [1 << (n - 1)] * n and on[1].tolist() == [0] * n
    assert np.array_equal(on[0], counts_of(want, n))
    assert np.array_equal(states[0], want) and states[1].tolist() == [[0]]
    assert closed.tolist() == [1, 1]
    assert eng.profile_stats['problems'] == 2 and eng.profile_stats['state_steps'] == lam + 1
    on2, _, closed2 = eng.attractor_profile([1, 0], [lam, 1], states=False)
    assert np.array_equal(on2, on) and closed2.tolist() == [1, 1]


@functools.lru_cache(maxsize=None)
def mixed_attractors():
    """the 128 attractors of MIXED from the reference, ordered so that neighbours differ in length"""
    _, net, space = compiled(MIXED)
    table = oracle_table(net, space, 128)             # (problems 0 .. 127: every identity assignment with the LFSR at 0 and at 1)
    assert len(table) == 128 and sorted(table.values()) == [1] * 64 + [1023] * 64       # guard
    short = sorted(k for k, l in table.items() if l == 1)
    long_ = sorted(k for k, l in table.items() if l == 1023)
    keys = [k for pair in zip(long_, short) for k in pair]
    return net, space, keys, [table[k] for k in keys]


def case_divergent_lanes(eng):
    net, space, keys, lengths = mixed_attractors()
    assert all(a != b for a, b in zip(lengths, lengths[1:]))
    eng.set_problem(net, space)
    on, states, closed = eng.attractor_profile(keys, lengths)
    assert closed.tolist() == [1] * 128
    for q in (0, 1, 64, 127):                                             # (the oracle walk of four, states_from of all)
        want, _ = oracle_walk(net, space, keys[q], lengths[q])
        assert np.array_equal(states[q], want) and np.array_equal(on[q], counts_of(want, 16))
    for q in range(128):
        assert np.array_equal(states[q], eng.states_from(keys[q], lengths[q] - 1))
        assert np.array_equal(on[q], counts_of(states[q], 16))
    at = 0
    for m in (1, 64, 63):                                                 # the same rows from three calls
        on_p, states_p, closed_p = eng.attractor_profile(keys[at:at + m], lengths[at:at + m])
        assert np.array_equal(on_p, on[at:at + m]) and closed_p.tolist() == [1] * m
        assert all(np.array_equal(a, b) for a, b in zip(states_p, states[at:at + m]))
        at += m
    assert at == 128


# n, seed, fixed nodes, a node with 9 predecessors -- seeds chosen on the CPU for the guard in case_width
WIDTH_CASES = {
    'n20': (20, 1, None, False),
    'n64': (64, 1, None, False),
    'n100': (100, 1, None, False),
    'n256': (256, 2, None, False),
    'n64_fixed': (64, 1, {20: '1', 41: '0'}, False),
    'n100_many_preds': (100, 6, None, True),
}


def case_width(eng, name):
    n, seed, fixed, many = WIDTH_CASES[name]
    _, net, space = compiled(random_text(n, seed, fixed=fixed, many_preds=many))
    table = oracle_table(net, space, 1 << 10)
    assert len(table) >= 2 and max(table.values()) > 1, table            # guard
    if fixed:                                                             # guard: the fixed nodes change the cycles
        _, net0, space0 = compiled(random_text(n, seed))
        assert oracle_table(net0, space0, 1 << 10) != table
    if many:
        assert max(np.diff(net.pred_offsets)) > 6
    eng.set_problem(net, space)
    merged, none, _ = run_attract_range(eng, 0, 1 << 10)
    assert none == 0 and {k: e[0] for k, e in merged.items()} == table
    keys = sorted(table)
    check_against_references(eng, net, space, keys, [table[k] for k in keys])


def case_batch_shapes(eng):
    n = 11
    preds, masks = [[i] for i in range(n)], [0b10] * n
    _, net, space = compiled(yaml_of(preds, masks, ['any'] * n))
    eng.set_problem(net, space)
    launches = {}
    for count in (100, 2048, 777):                                        # one workgroup, several, a ragged wave
        keys = [(k * 37) % 2048 for k in range(count)]                    # (37 is odd: distinct fixed points)
        assert len(set(keys)) == count
        on, states, closed = eng.attractor_profile(keys, [1] * count)
        want = np.array([[(k >> i) & 1 for i in range(n)] for k in keys], np.uint32)
        assert np.array_equal(on, want) and closed.tolist() == [1] * count
        assert [int(s[0, 0]) for s in states] == keys
        launches[count] = eng.profile_stats['kernel_launches']
        assert eng.profile_stats['problems'] == count and eng.profile_stats['state_steps'] == count
    assert launches[100] == launches[2048] == launches[777] == 1


def case_not_closed_and_errors(eng):
    net, space, keys, lengths = mixed_attractors()
    eng.set_problem(net, space)
    q = lengths.index(1023)
    want, back = oracle_walk(net, space, keys[q], 1022)
    assert words_to_code(back) != keys[q]                                 # guard: one step short of the cycle
    on, states, closed = eng.attractor_profile([keys[q], keys[q]], [1022, 1023])     # returns: not an error
    assert closed.tolist() == [0, 1]
    assert np.array_equal(states[0], want) and np.array_equal(on[0], counts_of(want, 16))
    # invalid arguments: refused by the host before anything is launched
    for bad_keys, bad_lengths, status in (([keys[q]], [0], ERR_INVALID), ([1 << 16], [1], ERR_INVALID),
                                          ([keys[q]], [1 << 30], ERR_STEP_LIMIT)):
        with pytest.raises(EngineError) as err:
            eng.attractor_profile(bad_keys, bad_lengths, states=False)
        assert err.value.status == status
    with pytest.raises(ValueError):
        eng.attractor_profile([1 << 64], [1])
    # before a network and a problem space are set: BSX_ERR_STATE, as from every bsx_run_* call
    import ctypes
    from boolsi_amd._lib import Stats, ptr
    with Engine(eng.device) as bare:
        one_key, one_length = np.array([1], np.uint64), np.array([1], np.uint64)
        rc = bare._lib.bsx_run_attractor_profile(bare._h, ptr(one_key), 1, ptr(one_length), 1, None, None, None, None,
                                                 ctypes.byref(Stats()))
        assert rc == ERR_STATE
    on, states, closed = eng.attractor_profile([], [])
    assert on.shape == (0, 16) and states == [] and len(closed) == 0


NARROW_CASES = ([('long10', lambda e: case_long_cycle(e, 10, 7)), ('long17', lambda e: case_long_cycle(e, 17, 14)),
                 ('divergent', case_divergent_lanes), ('batch', case_batch_shapes), ('not_closed', case_not_closed_and_errors)] +
                [(name, functools.partial(case_width, name=name)) for name in WIDTH_CASES])


@pytest.fixture(scope='module')
def eng():
    with Engine(0) as e:
        yield e


@pytest.mark.parametrize('name', [name for name, _ in NARROW_CASES])
def test_narrow(eng, name):
    assert not eng_is_wide_by_default()
    dict(NARROW_CASES)[name](eng)
    assert not eng.wide


def eng_is_wide_by_default():
    return os.environ.get('BSX_WIDE', '') == '1'


def test_narrow_cases_on_the_wide_family():
    # (the child takes 4 s on an MI355X, most of it start-up; it is ended after 60)
    env = dict(os.environ, BSX_WIDE='1')
    res = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    assert res.stdout.strip().endswith('wide family: {} cases ok'.format(len(NARROW_CASES)))


def test_handle_state_is_left_alone(eng):
    """the problem space and the cycle-state cache survive a profile call: the attract after it finds the table again and
    is as cheap as a repeat without a call in between, not as expensive as the first run on an empty cache"""
    _, net, space = compiled(random_text(64, 1, n_any=16))
    table = oracle_table(net, space, 1 << 12)
    assert len(table) >= 2                                                # guard
    eng.set_problem(net, space)
    first = eng.attract(0, 1 << 12)
    again = eng.attract(0, 1 << 12)
    keys = [int(words_to_code(r['key'])) for r in first.table]
    lengths = [int(r['length']) for r in first.table]
    assert dict(zip(keys, lengths)) == table
    eng.attractor_profile(keys, lengths)
    after = eng.attract(0, 1 << 12)
    order = lambda t: np.sort(t, order=['key', 'length'])
    assert np.array_equal(order(after.table), order(first.table)) and after.n_no_attractor == first.n_no_attractor
    cold, warm, got = (r.stats['executed_steps'] for r in (first, again, after))
    print('executed steps: first {} repeat {} after the profile call {}'.format(cold, warm, got))
    assert warm < cold                                                    # guard: the cache matters on this space
    assert got <= warm + (cold - warm) // 4                               # still warm (a dropped journal would cost `cold`)


# ---- wide family --------------------------------------------------------------------------------------------------------

# n -> (identity nodes, LFSR nodes in register order): the 7-node LFSR x^7 + x^6 + 1 (lambda = 127) and the identity block
# straddle 64-bit word boundaries above node 255.  At 257 the register itself runs 252 .. 256 (and on through two low
# nodes), so the single node of the ragged last word carries a changing bit, and the identity block crosses 63 / 64;
# lambda = 127 crosses eight flushes of the kernel's 15-step counters
WIDE_CASES = {
    257: ([60, 61, 62, 63, 64, 65, 66, 67, 68], [252, 253, 254, 255, 256, 10, 70]),        # 2^9 * 2 = 1024 attractors: L = 16, two groups
    577: ([510, 511, 512, 576], [316, 317, 318, 319, 320, 321, 322]),
    1024: ([1021, 1022, 1023, 0], [956, 957, 958, 959, 960, 961, 962]),
}


@functools.lru_cache(maxsize=None)
def wide_case(n):
    from wide_ref import WideRef, code_of
    identity, lfsr = WIDE_CASES[n]
    _, net, space = compiled(block_network(n, identity, lfsr, 6))
    ref = WideRef(net, space)
    assert lfsr_cycle_length(7, 6) == 127
    # keys: every identity assignment x (LFSR at zero -> fixed point, LFSR on its cycle -> lambda = 127); the cycle's
    # smallest code from the reference's own walk
    start = np.zeros((1, n), np.uint8)
    start[0, lfsr[0]] = 1
    S, codes = start, []
    for _ in range(127):
        codes.append(code_of(S[0]))
        S = ref.rules(S)
    assert np.array_equal(S, start) and len(set(codes)) == 127          # guard: a cycle of 127 states
    cycle_key = min(codes)
    keys, lengths = [], []
    for x in range(1 << len(identity)):
        part = sum(((x >> j) & 1) << node for j, node in enumerate(identity))
        keys += [part | cycle_key, part]
        lengths += [127, 1]
    # the reference walk of all attractors side by side, frozen after their length
    S = np.array([[(k >> i) & 1 for i in range(n)] for k in keys], np.uint8)
    L = np.array(lengths)
    states = [np.zeros((l, net.n_words), np.uint64) for l in lengths]
    counts = np.zeros((len(keys), n), np.uint32)
    for t in range(127):
        live = np.flatnonzero(L > t)
        packed = np.packbits(S[live], axis=1, bitorder='little')
        packed = np.pad(packed, ((0, 0), (0, net.n_words * 8 - packed.shape[1]))).view('<u8')
        for row, q in zip(packed, live):
            states[q][t] = row
        counts[live] += S[live]
        S[live] = ref.rules(S[live])
    assert np.array_equal(S, np.array([[(k >> i) & 1 for i in range(n)] for k in keys], np.uint8))     # guard: all closed
    return net, space, keys, lengths, states, counts


@pytest.mark.parametrize('n', sorted(WIDE_CASES))
def test_wide_family(eng, n):
    net, space, keys, lengths, states, counts = wide_case(n)
    if n == 257:
        assert len(keys) > 32 * 16 and len(keys) % (32 * 16) == 0
        keys, lengths, states, counts = keys[:-5], lengths[:-5], states[:-5], counts[:-5]      # a ragged second group
    eng.set_problem(net, space)
    assert eng.wide
    on, got, closed = eng.attractor_profile(keys, lengths)
    assert closed.tolist() == [1] * len(keys)
    assert np.array_equal(on, counts)
    assert all(np.array_equal(a, b) for a, b in zip(got, states))
    for q in (0, 1, len(keys) - 2, len(keys) - 1):
        assert np.array_equal(eng.states_from(keys[q], lengths[q] - 1), states[q])
    one = eng.profile_stats['kernel_launches']
    on2, none, closed2 = eng.attractor_profile(keys[:3], lengths[:3], states=False)
    assert none is None and np.array_equal(on2, counts[:3]) and closed2.tolist() == [1, 1, 1]
    assert eng.profile_stats['kernel_launches'] == one == 1
    # one step short of the cycle: not closed, not an error; a walk beyond the lock-step limit: refused by the host
    _, _, closed3 = eng.attractor_profile(keys[:2], [126, 1], states=False)
    assert closed3.tolist() == [0, 1]
    with pytest.raises(EngineError) as err:
        eng.attractor_profile(keys[:1], [1 << 24], states=False)
    assert err.value.status == ERR_STEP_LIMIT


# ---- host layer ---------------------------------------------------------------------------------------------------------

class CountingEngine(Engine):
    def __init__(self):
        super().__init__(0)
        self.n_states_from, self.profile_state_pointers = 0, []

    def states_from(self, state_code, n_steps):
        self.n_states_from += 1
        return super().states_from(state_code, n_steps)

    def _run_attractor_profile(self, keys, key_stride, lengths, n, on_counts, states, state_offsets, closed, stats):
        self.profile_state_pointers.append(states)
        return super()._run_attractor_profile(keys, key_stride, lengths, n, on_counts, states, state_offsets, closed, stats)


def test_attract_master_batches_the_table():
    cfg, net, space = compiled(MIXED)
    args = (cfg['origin simulation problem'], cfg['simulation problem variations'], cfg['incoming node lists'],
            cfg['truth tables'], float('inf'), float('inf'), cfg['total combination count'])
    with CountingEngine() as e:
        attractors, none, total, _ = attract_master(e, *args, with_states=True, with_activity=True)
        assert len(attractors) == 128 >= 50 and none == 0 and total == 1 << 16
        assert e.n_states_from == 0 and len(e.profile_state_pointers) == 1 and e.profile_state_pointers[0] is not None
        # the per-attractor loop this replaces, restated from states_from
        old = []
        for a in attractors:
            states = [decode_state(words_to_code(s), 16) for s in e.states_from(a.key, a.length - 1)]
            old.append(AggregatedAttractor(a.key, a.length, a.frequency, a.sum_l, a.sum_l2, states))
            assert a.states == states
            assert np.array_equal(a.activity, np.mean(np.array(states, dtype=float), axis=0))
        want, got = find_node_correlations(old), find_node_correlations(attractors)
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(want, got))
        # activity only: the states pointer passed down is null
        e.profile_state_pointers.clear()
        only, _, _, _ = attract_master(e, *args, with_states=False, with_activity=True)
        assert e.profile_state_pointers == [None] and all(a.states is None for a in only)
        assert all(np.array_equal(a.activity, b.activity) for a, b in zip(only, attractors))
        got = find_node_correlations(only)
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(want, got))
        # an attractor that does not close is an error naming the key
        from boolsi_amd.attract import profile_attractors
        bad = AggregatedAttractor(attractors[0].key, attractors[0].length + 1, 1, 0, 0)
        if attractors[0].length == 1:
            bad = next(AggregatedAttractor(a.key, a.length - 1, 1, 0, 0) for a in attractors if a.length > 1)
        with pytest.raises(RuntimeError, match=str(bad.key)):
            profile_attractors(e, [bad])


if __name__ == '__main__':
    # the child process of test_narrow_cases_on_the_wide_family: BSX_WIDE=1 lowers every network to the wide family
    assert eng_is_wide_by_default()
    with Engine(0) as engine:
        for case_name, case in NARROW_CASES:
            case(engine)
            assert engine.wide, case_name
            print(case_name, 'ok', flush=True)
    print('wide family: {} cases ok'.format(len(NARROW_CASES)))
