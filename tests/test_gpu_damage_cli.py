"""
`damage FILE --samples N --seed S -t T --flips 1,3 --histogram` end to end through the CLI: both CSVs equal, byte for
byte, text built here from the integers of the reference (damage_ref over samples 0 .. N - 1) by the formulas of the
command's documentation; then the usage errors, which need no engine.
"""
import faulthandler
import math

import pytest
from click.testing import CliRunner

from boolsi_amd.cli import cli

import damage_ref
from damage_cases import CASES, SEED, compiled
from test_gpu_cli import read, run_cli

pytestmark = pytest.mark.gpu
N, STEPS, FLIPS = 300, 12, (1, 3)


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def reference_texts(name):
    net, _, ref = compiled(name)
    n = net.n_nodes
    curve = ['flips,t,samples,mean_distance,normalized_distance,std_distance,merged_fraction']
    hist_lines = ['flips,t,distance,count']
    for h in FLIPS:
        sum_d, sum_d2, merged, hist = damage_ref.sums(damage_ref.distances(ref, SEED, 0, N, h, STEPS), n)
        assert sum_d[0] == h * N and any(s != h * N for s in sum_d) and 0 < merged[STEPS] < N
        for t in range(STEPS + 1):
            mean = sum_d[t] / N
            std = math.sqrt(max(0, N * sum_d2[t] - sum_d[t] * sum_d[t])) / N
            curve.append('{},{},{},{},{},{},{}'.format(h, t, N, repr(mean), repr(mean / n), repr(std), repr(merged[t] / N)))
            hist_lines += ['{},{},{},{}'.format(h, t, k, c) for k, c in enumerate(hist[t]) if c]
    return ('\r\n'.join(curve) + '\r\n').encode(), ('\r\n'.join(hist_lines) + '\r\n').encode()


@pytest.mark.parametrize('name', ['n300', 'n64'])
def test_damage_cli_writes_the_reference_curves(tmp_path, name):
    (tmp_path / 'net.yaml').write_text(CASES[name]())
    args = ['damage', str(tmp_path / 'net.yaml'), '--samples', str(N), '--seed', str(SEED), '-t', str(STEPS),
            '--flips', ','.join(str(h) for h in FLIPS)]
    curve, hist = reference_texts(name)
    out = run_cli(args + ['--histogram'], str(tmp_path / 'both'))
    assert 'Spreading damage over {} sampled pairs of states with seed {}'.format(N, SEED) in out
    assert read(tmp_path / 'both' / 'damage_spreading.csv') == curve
    assert read(tmp_path / 'both' / 'damage_histogram.csv') == hist
    if name == 'n64':
        run_cli(args, str(tmp_path / 'curve'))
        assert read(tmp_path / 'curve' / 'damage_spreading.csv') == curve
        assert not (tmp_path / 'curve' / 'damage_histogram.csv').exists()


def test_an_engine_error_is_logged_and_nothing_is_written(tmp_path):
    """More flips than free nodes: the CLI's policy for engine errors."""
    (tmp_path / 'net.yaml').write_text(CASES['n64']())
    out = run_cli(['damage', str(tmp_path / 'net.yaml'), '--samples', '10', '-t', '3', '--flips', '64'], str(tmp_path / 'out'))
    assert 'Exception caught' in out and 'n_flips' in out
    assert not (tmp_path / 'out' / 'damage_spreading.csv').exists()


@pytest.fixture
def model(tmp_path):
    path = tmp_path / 'net.yaml'
    path.write_text('nodes: [A, B]\nupdate rules: {A: B, B: A}\ninitial state: {A: any, B: any}\n')
    return str(path)


@pytest.mark.parametrize('args,words', [
    (['-t', '3', '--seed', '1'], ['--seed needs --samples']),
    (['-t', '3'], ['damage needs --samples']),
    (['--samples', '8'], ['-t']),
    (['--samples', '8', '-t', '3', '--flips', '1,x'], ['--flips', 'positive integers']),
    (['--samples', '8', '-t', '3', '--flips', '0'], ['--flips', 'positive integers']),
    (['--samples', '8', '-t', '65536'], ['-t']),
])
def test_usage_errors(model, tmp_path, args, words):
    res = CliRunner().invoke(cli, ['damage', model] + args + ['-o', str(tmp_path / 'out')])
    assert res.exit_code == 2, res.output
    assert 'Usage:' in res.output and all(w in res.output for w in words), res.output
    assert not (tmp_path / 'out').exists()
