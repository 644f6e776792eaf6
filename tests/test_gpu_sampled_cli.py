"""
`attract --samples N --seed S` end to end through the CLI: the CSVs equal, byte for byte, those the host layer
(boolsi_amd.output.output_attractors) writes from the reference's table of the same samples (sample_ref + wide_ref);
two ranks write what one writes; without --samples the command still reproduces the published example.
"""
import os

import numpy as np
import pytest

from boolsi_amd.attract import AggregatedAttractor
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text
from boolsi_amd.model import decode_state
from boolsi_amd.output import output_attractors

from sampled_cases import CASES, EXAMPLE2, compiled, expected, records
from test_gpu_cli import read, run_cli, run_cli_world
from wide_ref import code_of

pytestmark = pytest.mark.gpu
N, SEED = 4096, 7
CSVS = ('attractors.csv', 'attractor_summaries.csv')


def reference_csvs(name, out_dir):
    """The attractor CSVs from the reference's records of samples 0 .. N - 1, in the host layer's final order."""
    net, space, ref = compiled(name)
    table, none, _ = expected(records(name, 0, N, None, None, SEED))
    assert len(table) >= 2 and sum(e[1] for e in table.values()) + none == N
    attractors = []
    for key, (length, freq, s1, s2) in sorted(table.items(), key=lambda kv: (-kv[1][1], kv[0])):
        s = np.array([[(key >> i) & 1 for i in range(ref.n)]], np.uint8)
        states = []
        for _ in range(length):
            states.append(decode_state(code_of(s[0]), ref.n))
            s = np.where(ref.problem(0).fmask, ref.problem(0).fval, ref.rules(s))
        assert code_of(s[0]) == key
        attractors.append(AggregatedAttractor(key, length, freq, s1, s2, states=states))
    cfg = parse_input_text(CASES[name](), float('inf'), Mode.ATTRACT)
    _, fixed_nodes, _ = cfg['origin simulation problem']
    os.makedirs(out_dir)
    output_attractors(attractors, N - none, fixed_nodes, cfg['node names'], N, float('inf'), float('inf'), out_dir)


@pytest.mark.parametrize('name', ['n300', 'n64'])
def test_sampled_cli_writes_the_reference_tables_csvs(tmp_path, name):
    (tmp_path / 'net.yaml').write_text(CASES[name]())
    args = ['attract', str(tmp_path / 'net.yaml'), '--samples', str(N), '--seed', str(SEED), '-c']
    out = run_cli(args, str(tmp_path / 'one'))
    _, space, _ = compiled(name)
    assert 'Sampling {} initial conditions out of {} with seed {}.'.format(N, space.n_problems, SEED) in out
    assert 'Single process will be used to find attractors from {} initial conditions...'.format(N) in out
    reference_csvs(name, str(tmp_path / 'ref'))
    for f in CSVS:
        assert read(tmp_path / 'one' / f) == read(tmp_path / 'ref' / f), f
    if name == 'n64':
        outs = run_cli_world(args, str(tmp_path / 'two'))
        assert any('2 GPU' in o for o in outs), '\n'.join(outs)
        for f in CSVS:
            assert read(tmp_path / 'two' / f) == read(tmp_path / 'one' / f), f


def test_without_samples_the_published_example_is_reproduced(tmp_path):
    src = os.path.dirname(EXAMPLE2)
    out = run_cli(['attract', EXAMPLE2], str(tmp_path))
    assert 'Sampling' not in out and 'find attractors from 8 initial conditions' in out
    for f in ('attractors.csv', 'node_correlations.csv'):
        assert read(tmp_path / f) == read(os.path.join(src, f)), f
