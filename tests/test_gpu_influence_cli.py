"""
`influence FILE --samples N --seed S -t T --nodes ..` end to end through the CLI: both CSVs equal, byte for byte, text
built here from Engine.influence_sampled and text built from the integers of the reference (influence_ref over samples
0 .. N - 1) by the formulas of the command's documentation.
"""
import faulthandler

import pytest

from boolsi_amd import synth

import influence_ref
from influence_cases import CASES, SEED, compiled, sources_of
from test_gpu_cli import read, run_cli

pytestmark = pytest.mark.gpu
N, STEPS = 300, 12


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def texts(influence, merged, sources):
    """The two files from integer arrays [n_sources][STEPS][n] and [n_sources][STEPS], by the documented formulas."""
    matrix = ['source,t,target,count,probability']
    summary = ['source,t,samples,mean_damage,merged_fraction,reach']
    for s, v in enumerate(sources):
        for t in range(STEPS):
            cells = [int(c) for c in influence[s][t]]
            matrix += ['{},{},{},{},{}'.format(synth.node_name(v), t + 1, synth.node_name(i), c, repr(c / N))
                       for i, c in enumerate(cells) if c]
            summary.append('{},{},{},{},{},{}'.format(synth.node_name(v), t + 1, N, repr(sum(cells) / N), repr(int(merged[s][t]) / N),
                                                      sum(1 for c in cells if c)))
    return ('\r\n'.join(matrix) + '\r\n').encode(), ('\r\n'.join(summary) + '\r\n').encode()


def test_influence_cli_writes_the_reference_files(tmp_path):
    name = 'n300'
    net, space, ref = compiled(name)
    sources = list(sources_of(name))
    want = influence_ref.counts(ref, SEED, 0, N, sources, STEPS)
    assert int(want[0][:, 0].sum()) > 0 and ((want[1][:, -1] > 0) & (want[1][:, -1] < N)).any()
    (tmp_path / 'net.yaml').write_text(CASES[name]())
    # the names in reverse order: the files are in node order all the same
    out = run_cli(['influence', str(tmp_path / 'net.yaml'), '--samples', str(N), '--seed', str(SEED), '-t', str(STEPS),
                   '--nodes', ','.join(synth.node_name(v) for v in reversed(sources))], str(tmp_path / 'out'))
    assert 'Measuring the influence of {} nodes over {} sampled initial conditions with seed {}'.format(len(sources), N, SEED) in out
    sensitivity = sum(int(c) for row in want[0][:, 0] for c in row) / (N * len(sources))
    assert 'Average sensitivity of the network: {}.'.format(repr(sensitivity)) in out
    matrix, summary = texts(*want, sources)
    assert read(tmp_path / 'out' / 'influence_matrix.csv') == matrix
    assert read(tmp_path / 'out' / 'influence_summary.csv') == summary
    # the same files from the engine's arrays
    from boolsi_amd.engine import Engine
    with Engine(0) as eng:
        eng.set_problem(net, space)
        got, merged, _ = eng.influence_sampled(SEED, 0, N, sources, STEPS)
    assert texts(got, merged, sources) == (matrix, summary)


def test_the_default_is_every_free_node(tmp_path):
    name = 'n64'
    net, space, ref = compiled(name)
    sources = list(sources_of(name))
    assert len(sources) == 63
    (tmp_path / 'net.yaml').write_text(CASES[name]())
    run_cli(['influence', str(tmp_path / 'net.yaml'), '--samples', str(N), '--seed', str(SEED), '-t', str(STEPS)], str(tmp_path / 'out'))
    matrix, summary = texts(*influence_ref.counts(ref, SEED, 0, N, sources, STEPS), sources)
    assert read(tmp_path / 'out' / 'influence_matrix.csv') == matrix
    assert read(tmp_path / 'out' / 'influence_summary.csv') == summary
