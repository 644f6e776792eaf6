"""
Wide-state family (networks of up to 1024 nodes, include/bsx.h BSX_MAX_NODES_WIDE) at the sizes the CPU oracle
reaches, and by composition.  The oracle stops at 256 nodes; above that the family is pinned against the exact
numpy reference of tests/wide_ref.py by tests/test_gpu_wide_exact.py.  Here:
  * self-consistency: with BSX_WIDE=1 the golden vectors and the oracle's cases of the <= 256-node suite go through
    the wide kernels;
  * composition: a 512-node network made of two 256-node networks A and B with interleaved nodes, whose trajectories,
    lambda = lcm, mu = max and key follow from A and B on the oracle-pinned <= 256-node path;
  * the CLI on a 300-node network.
"""
import math
import os
import subprocess
import sys

import pytest

from boolsi_amd import _lib, synth
from boolsi_amd.attract import merge_tables
from boolsi_amd.compile import code_to_words, compile_problem, words_to_code
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text
from util import compile_case, contiguous_runs, load, t_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTRACT_CASES = [c for f in ('attract_toy.json', 'attract_examples.json', 'attract_synth.json') for c in load(f)]
# as in test_gpu_parity.py: the reference's -r solver is pinned only without a time cap
ATTRACT_CASES = [c for c in ATTRACT_CASES if c['storing_all_states'] or c['max_t'] is None]
# bsx_run_attract_wide takes 128-bit flat indices (as bsx_run_attract2)
ATTRACT_CASES = [c for c in ATTRACT_CASES if max(int(i) for i in c['indices']) < 1 << 128]


@pytest.fixture()
def eng():
    from boolsi_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture()
def wide_eng(monkeypatch):
    from boolsi_amd.engine import Engine
    monkeypatch.setenv('BSX_WIDE', '1')
    e = Engine(0)
    yield e
    e.close()


# ---- self-consistency at n <= 256 ----------------------------------------------------------------

@pytest.mark.parametrize('case', ATTRACT_CASES, ids=lambda c: c['name'])
def test_wide_attract_matches_golden(wide_eng, case):
    _, net, space = compile_case(case)
    wide_eng.set_problem(net, space)
    assert wide_eng.network_info()['lut_mode'] == _lib.LUT_WIDE
    idx = [int(i) for i in case['indices']]
    tables, none, steps = [], 0, 0
    for first, count, _ in contiguous_runs(idx):
        r = wide_eng.attract_wide(first, count, t_of(case['max_t']), t_of(case['max_len']))
        tables.append(r.table)
        none += r.n_no_attractor
        steps += r.stats['state_steps']
    merged = merge_tables(tables)
    order = sorted(merged.items(), key=lambda kv: (-kv[1][1], kv[0]))
    assert [[str(k), v[0], v[1], v[2], str(v[3])] for k, v in order] == case['aggregate']
    assert none == sum(1 for r in case['per_problem'] if not r[0])
    if case['storing_all_states']:
        assert steps == sum(r[4] for r in case['per_problem'])      # reference loop stop times


@pytest.mark.parametrize('case', load('target.json'), ids=lambda c: c['name'])
def test_wide_target_matches_golden(wide_eng, case):
    cfg, net, space = compile_case(case)
    wide_eng.set_problem(net, space)
    mask = code_to_words(sum(1 << n for n in cfg['target node set']), net.n_words)
    code = code_to_words(cfg['target substate code'], net.n_words)
    idx = [int(i) for i in case['indices']]
    rows = [[0, None] for _ in idx]
    for first, count, off in contiguous_runs(idx):
        hits, _ = wide_eng.target(first, count, t_of(case['max_t']), mask, code)
        for h in hits:
            rows[off + int(h['offset'])] = [1, int(h['t'])]
    for got, ref in zip(rows, case['per_problem']):
        assert got[0] == ref[0]
        if ref[0]:
            assert got[1] == ref[1]
    for i, states in case['trajectories'].items():
        trajs, _ = wide_eng.trajectories(int(i), [0], [len(states) - 1])
        assert [str(words_to_code(s)) for s in trajs[0]] == states


@pytest.mark.parametrize('case', load('simulate.json'), ids=lambda c: c['name'])
def test_wide_simulate_matches_golden(wide_eng, case):
    _, net, space = compile_case(case)
    wide_eng.set_problem(net, space)
    idx = [int(i) for i in case['indices']]
    for first, count, off in contiguous_runs(idx):
        traj, final, digest, st = wide_eng.simulate(first, count, case['max_t'])
        assert st['state_steps'] == count * case['max_t']
        for q in range(count):
            assert str(words_to_code(final[q])) == case['final'][off + q]
            assert str(int(digest[q])) == case['digest'][off + q]
            key = str(idx[off + q])
            if key in case['trajectories']:
                assert [str(words_to_code(s)) for s in traj[q]] == case['trajectories'][key]


def test_attract_wide_entry_point_equals_attract2_at_256_or_less(eng):
    cfg = parse_input_text(synth.network_yaml(100, 3, 77), 500, Mode.ATTRACT)
    net, space = compile_problem(cfg)
    eng.set_problem(net, space)
    a = eng.attract2(12345, 3000, 500)
    b = eng.attract_wide(12345, 3000, 500)
    assert a.n_no_attractor == b.n_no_attractor
    assert merge_tables([a.table]) == merge_tables([b.table])
    assert not b.table['key'][:, _lib.MAX_WORDS:].any()


# ---- composition at n = 512 ------------------------------------------------------------------------

N_ANY = 6


def _interleaved_yaml(a, b, init_a, init_b):
    """Node 2i = node i of A, node 2i + 1 = node i of B."""
    (pa, ma), (pb, mb) = a, b
    n = len(pa)
    out = ['nodes:'] + ['    - {}'.format(synth.node_name(i)) for i in range(2 * n)] + ['', 'update rules:']
    for i in range(n):
        out.append('    {}: {}'.format(synth.node_name(2 * i), synth.rule_text([2 * p for p in pa[i]], ma[i])))
        out.append('    {}: {}'.format(synth.node_name(2 * i + 1), synth.rule_text([2 * p + 1 for p in pb[i]], mb[i])))
    out += ['', 'initial state:']
    for i in range(n):
        out.append('    {}: {}'.format(synth.node_name(2 * i), init_a[i]))
        out.append('    {}: {}'.format(synth.node_name(2 * i + 1), init_b[i]))
    return '\n'.join(out) + '\n'


def _single_yaml(net, init):
    preds, masks = net
    out = ['nodes:'] + ['    - {}'.format(synth.node_name(i)) for i in range(len(preds))] + ['', 'update rules:']
    out += ['    {}: {}'.format(synth.node_name(i), synth.rule_text(preds[i], masks[i])) for i in range(len(preds))]
    out += ['', 'initial state:'] + ['    {}: {}'.format(synth.node_name(i), init[i]) for i in range(len(preds))]
    return '\n'.join(out) + '\n'


def _mix(code_a, code_b, n):
    v = 0
    for i in range(n):
        v |= ((code_a >> i) & 1) << (2 * i) | ((code_b >> i) & 1) << (2 * i + 1)
    return v


def test_composed_512_node_network(eng):
    n = 256
    net_a, net_b = synth.random_network(n, 2, 5101), synth.random_network(n, 2, 5102)
    bits_a, bits_b = synth.seeded_bits(n, 11), synth.seeded_bits(n, 12)
    init_a = ['any' if i < N_ANY else str(bits_a[i]) for i in range(n)]
    init_b = [str(x) for x in bits_b]
    count = 1 << N_ANY

    def load_space(text):
        cfg = parse_input_text(text, math.inf, Mode.ATTRACT)
        net, space = compile_problem(cfg)
        eng.set_problem(net, space)

    load_space(_single_yaml(net_b, init_b))
    rb = eng.attract(0, 1, per_problem=True).per_problem[0]
    assert rb['found']
    lam_b, mu_b = int(rb['length']), int(rb['trajectory_l'])
    load_space(_single_yaml(net_a, init_a))
    ra = eng.attract(0, count, per_problem=True).per_problem
    assert ra['found'].all()
    horizon = 40
    expected, traj_a = {}, {}
    for i in range(count):
        lam_a, mu_a = int(ra[i]['length']), int(ra[i]['trajectory_l'])
        lam, mu = lam_a * lam_b // math.gcd(lam_a, lam_b), max(mu_a, mu_b)
        ta, _ = eng.trajectories(i, [0], [max(mu + lam_a, horizon)])
        traj_a[i] = [words_to_code(s) for s in ta[0]]
        expected[i] = (lam, mu, lam_a)
    load_space(_single_yaml(net_b, init_b))
    longest = max(max(e[1] + lam_b, horizon) for e in expected.values())
    tb, _ = eng.trajectories(0, [0], [longest])
    traj_b = [words_to_code(s) for s in tb[0]]

    agg = {}
    for i in range(count):
        lam, mu, lam_a = expected[i]
        key = min(_mix(traj_a[i][mu + j % lam_a], traj_b[mu + j % lam_b], n) for j in range(lam))
        e = agg.setdefault(key, [lam, 0, 0, 0])
        e[1] += 1; e[2] += mu; e[3] += mu * mu

    load_space(_interleaved_yaml(net_a, net_b, init_a, init_b))
    assert eng.wide and eng.network_info()['state_words32'] == 16
    r = eng.attract_wide(0, count)
    assert r.n_no_attractor == 0
    assert merge_tables([r.table]) == agg
    trajs, _ = eng.trajectories(0, list(range(count)), [horizon] * count)
    for i in range(count):
        assert [words_to_code(s) for s in trajs[i]] == [_mix(traj_a[i][t], traj_b[t], n) for t in range(horizon + 1)]
    traj, final, digest, _ = eng.simulate(0, count, horizon)
    assert [words_to_code(f) for f in final] == [_mix(traj_a[i][horizon], traj_b[horizon], n) for i in range(count)]
    # the old attract entry points refuse wide networks and name the new one
    with pytest.raises(_lib.EngineError, match='bsx_run_attract_wide') as e:
        eng.attract2(0, count)
    assert e.value.status == _lib.ERR_UNSUPPORTED


# ---- bsx_run_target's capacity check on a wide engine ----------------------------------------------

def test_wide_target_list_at_and_below_its_capacity(eng):
    """The 300-node copy ring of test_gpu_wide_reduce.py, 2^10 problems: with cap = hits the list is the exact
    reference's, with one less the call returns BSX_ERR_TABLE_FULL and the engine goes on working."""
    from test_gpu_wide_reduce import RING_YAML
    from wide_ref import WideRef
    net, space = compile_problem(parse_input_text(RING_YAML, math.inf, Mode.ATTRACT))
    eng.set_problem(net, space)
    assert eng.wide
    first, count, max_t, nodes = 0, 1 << 10, 150, (100, 103)
    code = sum(1 << i for i in nodes)
    ref = [(q, t) for q, (reached, t) in enumerate(WideRef(net, space).target(range(first, first + count), max_t, nodes, code))
           if reached]
    assert 1 < len(ref) < count
    words = code_to_words(code, net.n_words)
    listed = lambda hits: [(int(h['offset']), int(h['t'])) for h in hits]
    assert listed(eng.target(first, count, max_t, words, words, cap=len(ref))[0]) == ref
    with pytest.raises(_lib.EngineError) as e:
        eng.target(first, count, max_t, words, words, cap=len(ref) - 1)
    assert e.value.status == _lib.ERR_TABLE_FULL
    assert listed(eng.target(first, count, max_t, words, words)[0]) == ref


# ---- CLI at n = 300 --------------------------------------------------------------------------------

def test_cli_on_a_300_node_network(tmp_path):
    n = 300
    init = {i: str(b) for i, b in enumerate(synth.seeded_bits(n, 3))}
    for i in range(4):
        init[i] = 'any'
    text = synth.network_yaml(n, 2, 3003, initial=init, perturbations={7: {'1': '2'}})
    path = tmp_path / 'net300.yaml'
    path.write_text(text)
    for cmd in (['simulate', str(path), '-t', '5'], ['attract', str(path)]):
        out_dir = tmp_path / cmd[0]
        res = subprocess.run([sys.executable, '-m', 'boolsi_amd'] + cmd + ['-o', str(out_dir)], cwd=ROOT,
                             capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout + res.stderr
        files = os.listdir(out_dir)
        assert files, res.stdout + res.stderr
    sims = [f for f in os.listdir(tmp_path / 'simulate') if f.startswith('simulations')]
    assert sims


# ---- the oracle's n <= 256 cases through the wide kernels (BSX_WIDE=1): nodes with more than 6 predecessors,
#      fixed-node and perturbation variations (per-trajectory masks, T_p freeze), target summary ------------------

VARIATIONS_YAML = synth.network_yaml(40, 2, 77, initial={i: str(i & 1) for i in range(14, 40)},
                                     fixed={3: 'any?', 17: '0?', 21: 'any'},
                                     perturbations={5: {'1': '2, 6-7', 'any?': '9'}, 30: {'0?': '3'}})
ORACLE_CASES = [       # name, YAML, parse mode, [(first, count, max_t, max_len)]
    ('k9_n24', synth.network_yaml(24, 9, 924), Mode.ATTRACT, [(0, 1 << 12, 2000, None), (12345, 3000, 50, 4)]),
    ('k12_n20', synth.network_yaml(20, 12, 2012), Mode.ATTRACT, [(0, 1 << 13, 5000, None)]),
    ('variations_n40', VARIATIONS_YAML, Mode.SIMULATE, [(0, 1 << 15, 4096, None), (123456, 5000, 12, 2),
                                                        (-40000, 40000, 4096, None)]),
]


def _oracle_setup(eng, text, mode, max_t):
    from oracle.cpu_oracle import Oracle
    cfg = parse_input_text(text, max_t, mode)
    net, space = compile_problem(cfg)
    eng.set_problem(net, space)
    assert eng.wide
    return cfg, net, space, Oracle(net, space)


@pytest.mark.parametrize('name,text,mode,runs', ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_wide_attract_vs_oracle(wide_eng, name, text, mode, runs):
    from oracle.cpu_oracle import key_int as okey
    _, net, space, orc = _oracle_setup(wide_eng, text, mode, max(r[2] for r in runs))
    for first, count, max_t, max_len in runs:
        first = first % space.n_problems
        r = wide_eng.attract_wide(first, count, max_t, t_of(max_len))
        pp, _, none, steps = orc.attract(first, count, max_t, max_len, True, n_threads=8)
        ref = {}
        for q in range(count):
            if pp[q]['found']:
                e = ref.setdefault(okey(pp[q]['key']), [int(pp[q]['length']), 0, 0, 0])
                tl = int(pp[q]['trajectory_l'])
                e[1] += 1; e[2] += tl; e[3] += tl * tl
        assert merge_tables([r.table]) == ref
        assert r.n_no_attractor == none
        assert r.stats['state_steps'] == steps


@pytest.mark.parametrize('name,text,mode,runs', ORACLE_CASES, ids=[c[0] for c in ORACLE_CASES])
def test_wide_simulate_and_target_vs_oracle(wide_eng, name, text, mode, runs):
    _, net, space, orc = _oracle_setup(wide_eng, text, mode, 64)
    first, count, max_t = 4321 % space.n_problems, min(3000, space.n_problems), 40
    first = min(first, space.n_problems - count)
    traj, final, digest, _ = wide_eng.simulate(first, count, max_t)
    otraj, ofinal, odigest, _ = orc.simulate(first, count, max_t)
    assert (traj == otraj).all() and (final == ofinal).all() and (digest == odigest).all()
    # target: a substate of five nodes, from a state that some trajectories pass through
    nodes = [1, 4, 7, 10, 13]
    mask = code_to_words(sum(1 << i for i in nodes), net.n_words)
    s = words_to_code(otraj[7][9])
    code = code_to_words(sum(((s >> i) & 1) << i for i in nodes), net.n_words)
    hits, _ = wide_eng.target(first, count, max_t, mask, code)
    pp, _ = orc.target(first, count, max_t, mask, code, n_threads=8)
    ref = [(q, int(pp[q]['t_stop'])) for q in range(count) if pp[q]['reached']]
    assert ref and [(int(h['offset']), int(h['t'])) for h in hits] == ref
    n_hits, hist, listed, _ = wide_eng.target_summary(first, count, max_t, mask, code, hist_bins=8, cap=5)
    assert n_hits == len(ref)
    assert [(int(h['offset']), int(h['t'])) for h in listed] == ref[:5]
    assert hist.tolist() == [sum(1 for _, t in ref if t == b) for b in range(7)] + [sum(1 for _, t in ref if t >= 7)]


# ---- step limit: a large finite max_t on a network without short cycles ends in BSX_ERR_STEP_LIMIT ----------

def test_wide_step_limit_with_large_finite_max_t(eng, monkeypatch):
    monkeypatch.setenv('BSX_WIDE_STEP_LIMIT', '4096')
    n = 300
    init = {i: ('any' if i < 8 else str(b)) for i, b in enumerate(synth.seeded_bits(n, 5))}
    cfg = parse_input_text(synth.network_yaml(n, 3, 300 * 1000 + 3, initial=init), 1000, Mode.ATTRACT)
    net, space = compile_problem(cfg)
    eng.set_problem(net, space)
    r = eng.attract_wide(0, 256, 200)               # a cap within the limit: an answer, no error
    assert r.n_no_attractor > 0
    for max_t in (10 ** 12, (1 << 63) + 5, math.inf):
        with pytest.raises(_lib.EngineError) as e:
            eng.attract_wide(0, 256, max_t)
        assert e.value.status == -6                 # BSX_ERR_STEP_LIMIT, not a table of "no attractor"
    mask = code_to_words((1 << n) - 1, net.n_words)
    code = code_to_words((1 << n) - 1, net.n_words)   # every node on: a state this network does not reach
    with pytest.raises(_lib.EngineError) as e:
        eng.target(0, 256, 10 ** 12, mask, code)
    assert e.value.status == -6
