"""
`target --samples N --seed S` and `simulate --samples N --seed S -t T` end to end: the CSVs are, byte for byte, what
output_simulations writes from Simulations built with the reference alone (sample_ref.sample_indices -> WideRef.target /
.trajectories, labels from problem_from_index on the flat index).
"""
import functools
import os

import pytest

from boolsi_amd import synth
from boolsi_amd.batching import create_numeral_system_from_variations, problem_from_index
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text
from boolsi_amd.model import decode_state
from boolsi_amd.output import output_simulations
from boolsi_amd.simulate import Simulation

import sample_ref
from sampled_cases import CASES, SEED, compiled
from sampled_target_cases import TARGETS
from test_gpu_cli import EXAMPLES, read, run_cli, run_cli_world

pytestmark = pytest.mark.gpu
N_TARGET, N_SIMULATE, SIM_T = 4096, 64, 6
FILES = ('simulation_summaries.csv', 'simulations.csv')


def target_yaml(name):
    """The case's input with its target substate (sampled_target_cases.TARGETS); every other node 'any'."""
    nodes, code, _ = TARGETS[name]
    n = compiled(name)[0].n_nodes
    lines = ['', 'target state:'] + ['    {}: {}'.format(synth.node_name(i), (code >> i) & 1 if i in nodes else 'any') for i in range(n)]
    return CASES[name]() + '\n'.join(lines) + '\n'


def simulations(name, cfg, indices, t_len):
    """Reference Simulations of the problems `indices`, s(0 .. t_len[q])."""
    net, space, ref = compiled(name)
    origin, variations = cfg['origin simulation problem'], cfg['simulation problem variations']
    numeral_system = create_numeral_system_from_variations(variations)
    out = []
    for index, codes in zip(indices, ref.trajectories(indices, t_len)):
        _, fixed_nodes, perturbed = problem_from_index(index, origin, variations, numeral_system)
        out.append(Simulation([decode_state(c, net.n_nodes) for c in codes], fixed_nodes, perturbed))
    return out


@functools.lru_cache(maxsize=None)
def expect_target(name):
    net, space, ref = compiled(name)
    nodes, code, _ = TARGETS[name]
    idx = sample_ref.sample_indices(space, SEED, range(N_TARGET))
    res = ref.target(idx, None, nodes, code)
    hits = [(q, t) for q, (reached, t) in enumerate(res) if reached]
    assert 5 < len(hits) < N_TARGET and len({t for _, t in hits}) >= 2
    return idx, hits


def write_reference(name, cfg, indices, t_len, where):
    os.makedirs(where)
    output_simulations(simulations(name, cfg, indices, t_len), cfg['node names'], str(where))


@pytest.mark.parametrize('name', ['n300', 'n64'])
def test_target_samples(tmp_path, name):
    idx, hits = expect_target(name)
    text = target_yaml(name)
    path = tmp_path / 'net.yaml'
    path.write_text(text)
    cfg = parse_input_text(text, float('inf'), Mode.TARGET)
    assert cfg['target node set'] == set(TARGETS[name][0]) and cfg['target substate code'] == TARGETS[name][1]
    args = ['target', str(path), '--samples', str(N_TARGET), '--seed', str(SEED)]
    out = run_cli(args, str(tmp_path / 'all'))
    assert 'Sampling {} initial conditions out of {} with seed {}.'.format(N_TARGET, cfg['total combination count'], SEED) in out
    assert 'perform {} simulations and find all'.format(N_TARGET) in out
    assert 'Only {} simulations reach target state.'.format(len(hits)) in out
    write_reference(name, cfg, [idx[q] for q, _ in hits], [t for _, t in hits], tmp_path / 'ref_all')
    for f in FILES:
        assert read(tmp_path / 'all' / f) == read(tmp_path / 'ref_all' / f), f
    # -n 5: the first five in sample order
    out = run_cli(args + ['-n', '5'], str(tmp_path / 'five'))
    assert 'find 5 that reach target states' in out and 'At least 5 simulations reach target state.' in out
    write_reference(name, cfg, [idx[q] for q, _ in hits[:5]], [t for _, t in hits[:5]], tmp_path / 'ref_five')
    for f in FILES:
        assert read(tmp_path / 'five' / f) == read(tmp_path / 'ref_five' / f), f
    if name == 'n64':           # two ranks write what one writes, with and without -n
        for extra, one in (([], 'all'), (['-n', '5'], 'five')):
            outs = run_cli_world(args + extra, str(tmp_path / ('world_' + one)))
            assert any('2 GPU' in o for o in outs), '\n'.join(outs)
            for f in FILES:
                assert read(tmp_path / ('world_' + one) / f) == read(tmp_path / one / f), (one, f)


@pytest.mark.parametrize('name', ['n300', 'n64'])
def test_simulate_samples(tmp_path, name):
    net, space, ref = compiled(name)
    text = CASES[name]()
    path = tmp_path / 'net.yaml'
    path.write_text(text)
    cfg = parse_input_text(text, SIM_T, Mode.SIMULATE)
    idx = sample_ref.sample_indices(space, SEED, range(N_SIMULATE))
    assert len(set(idx)) == N_SIMULATE
    args = ['simulate', str(path), '-t', str(SIM_T), '--samples', str(N_SIMULATE), '--seed', str(SEED)]
    out = run_cli(args, str(tmp_path / 'one'))
    assert 'Sampling {} initial conditions out of {} with seed {}.'.format(N_SIMULATE, cfg['total combination count'], SEED) in out
    assert 'perform {} simulations'.format(N_SIMULATE) in out
    write_reference(name, cfg, idx, [SIM_T] * N_SIMULATE, tmp_path / 'ref')
    for f in FILES:
        assert read(tmp_path / 'one' / f) == read(tmp_path / 'ref' / f), f
    if name == 'n64':
        outs = run_cli_world(args, str(tmp_path / 'world'))
        assert any('2 GPU' in o for o in outs), '\n'.join(outs)
        for f in FILES:
            assert read(tmp_path / 'world' / f) == read(tmp_path / 'one' / f), f


def test_target_without_samples_still_reproduces_a_published_example(tmp_path):
    src = os.path.join(EXAMPLES, 'output4_example3')
    out = run_cli(['target', os.path.join(src, 'example3.yaml')], str(tmp_path))
    assert 'Sampling' not in out
    for f in FILES:
        assert read(tmp_path / f) == read(os.path.join(src, f)), f
