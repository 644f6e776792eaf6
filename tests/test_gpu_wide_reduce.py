"""
Device-side reduction of the wide-state family (csrc/bsx_wide_reduce.hip): bsx_run_attract_wide folds the kernel's
per-problem records into an HBM table on the device, bsx_run_target_summary counts and bins hit times there.
Pinned by
  * the CPU oracle at n <= 256 (BSX_WIDE=1), over ranges that span several kernel launches;
  * a closed form above 256 nodes: a ring of 300 nodes in which node i copies node i - 1, so that every trajectory
    is a rotation of its initial state;
  * the host-side aggregation the library had before (BSX_WIDE_HOST_REDUCE=1), record for record and in order.
Every run makes its own engine after the environment is set, the way the wide_eng fixture of
test_gpu_wide_family.py does.
"""
import functools
import math

import pytest

from boolsi_amd import _lib, synth
from boolsi_amd.attract import merge_tables
from boolsi_amd.compile import code_to_words, compile_problem, words_to_code
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text

pytestmark = pytest.mark.gpu
ERR_TABLE_FULL = -5


@functools.lru_cache(maxsize=None)
def compiled(text, mode, max_t):
    """Parsed and lowered once per input: both legs of a test share it."""
    return compile_problem(parse_input_text(text, max_t, mode))


def run(monkeypatch, text, mode, max_t, fn, host=False, wide=False, chunk=None):
    """fn(engine, net, space) on a fresh engine made under the given environment."""
    from boolsi_amd.engine import Engine
    net, space = compiled(text, mode, max_t)
    with monkeypatch.context() as mp:
        for name, val in (('BSX_WIDE', '1' if wide else None), ('BSX_WIDE_HOST_REDUCE', '1' if host else None),
                          ('BSX_WIDE_CHUNK', str(chunk) if chunk else None)):
            if val is None:
                mp.delenv(name, raising=False)
            else:
                mp.setenv(name, val)
        eng = Engine(0)
        try:
            eng.set_problem(net, space)
            assert eng.wide
            return fn(eng, net, space)
        finally:
            eng.close()


def yaml_of(preds, masks, init):
    out = ['nodes:'] + ['    - {}'.format(synth.node_name(i)) for i in range(len(preds))] + ['', 'update rules:']
    out += ['    {}: {}'.format(synth.node_name(i), synth.rule_text(preds[i], masks[i])) for i in range(len(preds))]
    out += ['', 'initial state:'] + ['    {}: {}'.format(synth.node_name(i), init[i]) for i in range(len(preds))]
    return '\n'.join(out) + '\n'


def rows(table):
    """Records as plain tuples, in the order the library returned them."""
    return [(tuple(r['key'].tolist()), int(r['length']), tuple(r['count'].tolist()), tuple(r['sum_l'].tolist()),
             tuple(r['sum_l2'].tolist())) for r in table]


# ---- attract 1: the oracle at n = 20 over 3 * 2^18 + 7 problems ----------------------------------------------

def test_attract_matches_oracle_across_chunks_and_waits_once(monkeypatch):
    from oracle.cpu_oracle import Oracle
    text = synth.network_yaml(20, 2, 2020)                  # every node 'any': 2^20 problems
    first, count, max_t = 12345, 3 * (1 << 18) + 7, 2000

    def device(eng, net, space):
        one = eng.attract_wide(first, 1 << 18, max_t)
        return one, eng.attract_wide(first, count, max_t), Oracle(net, space).attract(first, count, max_t, None, True,
                                                                                       per_problem=False, n_threads=8)

    one, r, (_, otable, onone, osteps) = run(monkeypatch, text, Mode.ATTRACT, max_t, device, wide=True)
    assert merge_tables([r.table]) == merge_tables([otable])
    assert r.n_no_attractor == onone
    assert r.stats['state_steps'] == osteps
    assert r.stats['dominant_launches'] == 4 and one.stats['dominant_launches'] == 1
    print('host_syncs', one.stats['host_syncs'], r.stats['host_syncs'], 'launches', r.stats['kernel_launches'])
    assert r.stats['host_syncs'] == one.stats['host_syncs']     # the host waits once, however many chunks
    h = run(monkeypatch, text, Mode.ATTRACT, max_t, lambda eng, net, space: eng.attract_wide(first, count, max_t),
            wide=True, host=True)
    assert rows(h.table) == rows(r.table) and h.n_no_attractor == r.n_no_attractor
    assert h.stats['host_syncs'] == 4                           # the old path: one wait per chunk


# ---- the 300-node ring ---------------------------------------------------------------------------------------

RING_N, RING_ANY = 300, 12
RING_MASK = (1 << RING_N) - 1
RING_YAML = yaml_of([[(i - 1) % RING_N] for i in range(RING_N)], [0b10] * RING_N,
                    ['any' if i < RING_ANY else '0' for i in range(RING_N)])


def rot(v, s):
    """State after s steps: node i takes the value of node i - 1."""
    s %= RING_N
    return ((v << s) | (v >> (RING_N - s))) & RING_MASK


@pytest.fixture(scope='module')
def ring_table():
    """Problem p starts from state code p (bit i = node i); mu = 0, T_p = 0.
    -> ({key: [length, count, sum l, sum l^2]}, key of every problem)"""
    agg, keys = {}, []
    for p in range(1 << RING_ANY):
        key = min(rot(p, s) for s in range(RING_N))
        keys.append(key)
        lam = next(s for s in range(1, RING_N + 1) if rot(p, s) == p)
        e = agg.setdefault(key, [lam, 0, 0, 0])
        assert e[0] == lam
        e[1] += 1
    assert len(agg) == (1 << (RING_ANY - 1)) + 1 and len({e[1] for e in agg.values()}) > 1
    assert all(e[0] == (RING_N if k else 1) for k, e in agg.items())
    return agg, keys


@pytest.mark.parametrize('host', [False, True], ids=['device', 'host'])
def test_ring_attract_closed_form(monkeypatch, ring_table, host):
    count = 1 << RING_ANY
    ring_table = ring_table[0]

    def go(eng, net, space):
        # the state encoding the closed form relies on: problem p starts at code p and rotates
        trajs, _ = eng.trajectories(0, [0b101101, count - 1], [7, 7])
        for p, tr in zip((0b101101, count - 1), trajs):
            assert [words_to_code(s) for s in tr] == [rot(p, t) for t in range(8)]
        assert words_to_code(code_to_words(rot(5, 298), net.n_words)) == rot(5, 298)
        exact = eng.attract_wide(0, count, math.inf, cap=len(ring_table))       # cap == number of attractors
        with pytest.raises(_lib.EngineError) as e:
            eng.attract_wide(0, count, math.inf, cap=100)
        assert e.value.status == ERR_TABLE_FULL
        short = eng.attract_wide(0, count, RING_N - 1)
        return exact, short

    exact, short = run(monkeypatch, RING_YAML, Mode.ATTRACT, math.inf, go, host=host, chunk=1024)
    assert exact.stats['dominant_launches'] == 4
    assert merge_tables([exact.table]) == ring_table
    assert exact.n_no_attractor == 0
    keys = [words_to_code(k) for k in exact.table['key']]
    assert keys == sorted(keys, key=lambda k: [(k >> (64 * w)) & (2 ** 64 - 1) for w in range(16)])
    assert merge_tables([short.table]) == {0: [1, 1, 0, 0]}     # lambda = 300 needs t = 300
    assert short.n_no_attractor == count - 1


# ---- attract 4: more distinct keys in a tile than its LDS table holds ------------------------------------------

@pytest.mark.parametrize('chunk', [None, 512], ids=['one_launch', 'chunk512'])
def test_ring_lds_table_overflow(monkeypatch, ring_table, chunk):
    # 1024 consecutive problems hold at least 512 distinct attractors; the workgroup's table has 128 entries
    first, count = 37, (1 << RING_ANY) - 37 - 5
    go = lambda eng, net, space: eng.attract_wide(first, count)
    d = run(monkeypatch, RING_YAML, Mode.ATTRACT, math.inf, go, chunk=chunk)
    h = run(monkeypatch, RING_YAML, Mode.ATTRACT, math.inf, go, chunk=chunk, host=True)
    assert rows(d.table) == rows(h.table) and d.n_no_attractor == h.n_no_attractor == 0
    want = {}
    for key in ring_table[1][first:first + count]:
        want.setdefault(key, [ring_table[0][key][0], 0, 0, 0])[1] += 1
    assert merge_tables([d.table]) == want


# ---- attract 3: few attractors, heavy duplication (the LDS combining path) -------------------------------------

def bench_yaml(n, k, n_any=20, extra_preds=0, perturbations=None):
    """The networks of tools/bench_wide.py; extra_preds > 0 gives node 5 that many predecessors more."""
    preds, masks = synth.random_network(n, k, 1000 * n + k)
    if extra_preds:
        import random
        rng = random.Random(n)
        preds[5] = sorted(rng.sample(range(n), k + extra_preds))
        masks[5] = rng.getrandbits(1 << (k + extra_preds))
    init = ['any' if i < n_any else str(b) for i, b in enumerate(synth.seeded_bits(n, n + k))]
    text = yaml_of(preds, masks, init)
    if perturbations:
        text += '\nperturbations:\n'
        for i, by_state in perturbations.items():
            text += '    {}:\n'.format(synth.node_name(i))
            text += ''.join("        '{}': '{}'\n".format(s, times) for s, times in by_state.items())
    return text


DUP_CASES = [       # name, arguments of bench_yaml, parse mode
    # K = 2 networks settle within max_t = 512: 2^16 problems on a handful of attractors (the LDS combining path)
    ('n300_k2', dict(n=300, k=2), Mode.ATTRACT),
    ('n512_k2', dict(n=512, k=2), Mode.ATTRACT),
    ('n1024_k2_wide_node', dict(n=1024, k=2, extra_preds=6), Mode.ATTRACT),
    # T_p differs inside a group: 6 variants of 2^14 initial states each
    ('n300_k2_pert_variations', dict(n=300, k=2, n_any=14, perturbations={5: {'any?': '3'}, 30: {'0?': '2'}}), Mode.SIMULATE),
    # chaotic at K = 3 and 6: whatever they find within max_t = 512 (possibly nothing), both paths agree
    ('n512_k3', dict(n=512, k=3), Mode.ATTRACT),
    ('n1024_k6_wide_node', dict(n=1024, k=6, extra_preds=3), Mode.ATTRACT),
]
MAX_FEW = 64        # "few": far fewer attractors than the 2^16 problems, so nearly every record is a duplicate


@pytest.mark.parametrize('name,args,mode', DUP_CASES, ids=[c[0] for c in DUP_CASES])
def test_device_table_equals_host_table(monkeypatch, name, args, mode):
    count, max_t = 1 << 16, 512
    text = bench_yaml(**args)
    go = lambda eng, net, space: eng.attract_wide(0, count, max_t)
    d = run(monkeypatch, text, mode, max_t, go)
    h = run(monkeypatch, text, mode, max_t, go, host=True)
    print(name, 'attractors', len(d.table), 'none', d.n_no_attractor, 'host_syncs', d.stats['host_syncs'], h.stats['host_syncs'])
    assert rows(d.table) == rows(h.table)
    assert d.n_no_attractor == h.n_no_attractor
    assert d.stats['state_steps'] == h.stats['state_steps'] and d.stats['executed_steps'] == h.stats['executed_steps']
    assert sum(int(r['count'][0]) for r in d.table) + d.n_no_attractor == count
    if args['k'] == 2:
        assert 0 < len(d.table) <= MAX_FEW and d.n_no_attractor < count // 2
    if 'pert' in name:
        assert any(int(r['sum_l'][0]) for r in d.table)


# ---- target ----------------------------------------------------------------------------------------------------

def summaries(eng, first, count, max_t, mask, code, n_ref):
    out = {}
    for bins in (1, 4, max_t + 2):
        for cap in (0, 3, n_ref):
            n_hits, hist, listed, _ = eng.target_summary(first, count, max_t, mask, code, hist_bins=bins, cap=cap)
            out[bins, cap] = (n_hits, hist.tolist(), [(int(x['offset']), int(x['t'])) for x in listed])
    return out


def check_summaries(got, ref, max_t):
    for (bins, cap), (n_hits, hist, listed) in got.items():
        assert n_hits == len(ref)
        assert hist == [sum(1 for _, t in ref if (t == b if b < bins - 1 else t >= b)) for b in range(bins)]
        assert listed == ref[:cap]


VARIATIONS_YAML = synth.network_yaml(40, 2, 77, initial={i: str(i & 1) for i in range(14, 40)},
                                     fixed={3: 'any?', 17: '0?', 21: 'any'},
                                     perturbations={5: {'1': '2, 6-7', 'any?': '9'}, 30: {'0?': '3'}})
TARGET_CASES = [('k9_n24', synth.network_yaml(24, 9, 924), Mode.ATTRACT), ('variations_n40', VARIATIONS_YAML, Mode.SIMULATE)]


@pytest.mark.parametrize('name,text,mode', TARGET_CASES, ids=[c[0] for c in TARGET_CASES])
def test_target_summary_vs_oracle(monkeypatch, name, text, mode):
    from oracle.cpu_oracle import Oracle
    first, count, max_t = 4321, 5000, 40        # three launches at the smallest chunk (2048 problems at L = 64)
    nodes = [1, 4, 7, 10, 13]

    def prepare(eng, net, space):
        orc = Oracle(net, space)
        otraj, _, _, _ = orc.simulate(first, 16, max_t)
        s = words_to_code(otraj[7][9])          # a state that some trajectories pass through
        mask = code_to_words(sum(1 << i for i in nodes), net.n_words)
        code = code_to_words(sum(((s >> i) & 1) << i for i in nodes), net.n_words)
        pp, _ = orc.target(first, count, max_t, mask, code, n_threads=8)
        ref = [(q, int(pp[q]['t_stop'])) for q in range(count) if pp[q]['reached']]
        return mask, code, ref, summaries(eng, first, count, max_t, mask, code, len(ref))

    mask, code, ref, dev = run(monkeypatch, text, mode, 64, prepare, wide=True, chunk=1024)
    assert len(ref) > 3 and len({t for _, t in ref}) > 1
    check_summaries(dev, ref, max_t)
    host = run(monkeypatch, text, mode, 64, lambda eng, net, space: summaries(eng, first, count, max_t, mask, code, len(ref)),
               wide=True, chunk=1024, host=True)
    assert host == dev


def test_ring_target_closed_form(monkeypatch):
    # target: nodes 100 and 103 on.  s_t(i) = s_0(i - t), so the first hit is at t = 100 - a for the largest a <= 8
    # with bits a and a + 3 of p set (t = 89 .. 100); the ring comes round again only at t = 300 > max_t
    first, count, max_t = 33, 4019, 150         # not a multiple of the group of 512; four launches at chunk 1024
    ref = []
    for q in range(count):
        p = first + q
        a = max((a for a in range(9) if (p >> a) & 1 and (p >> (a + 3)) & 1), default=None)
        if a is not None:
            ref.append((q, 100 - a))
    for q, t in ref[:3] + ref[-3:]:
        assert all(((rot(first + q, u) >> 100) & (rot(first + q, u) >> 103) & 1) == (u == t) for u in range(t + 1))

    def go(eng, net, space):
        mask = code_to_words((1 << 100) | (1 << 103), net.n_words)
        return summaries(eng, first, count, max_t, mask, mask, len(ref))

    dev = run(monkeypatch, RING_YAML, Mode.ATTRACT, math.inf, go, chunk=1024)
    check_summaries(dev, ref, max_t)
    assert run(monkeypatch, RING_YAML, Mode.ATTRACT, math.inf, go, chunk=1024, host=True) == dev
