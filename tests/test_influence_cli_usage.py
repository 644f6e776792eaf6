"""
`influence`: the option checks and the source order, which need no GPU.  Usage errors are raised before the output directory
is made or an engine opened (click's runner); the sources come in node order whatever order --nodes names them in, and the
default is every node the input does not fix.  Then the rows of the two CSVs from hand-made integers.
"""
import numpy as np
import pytest
from click.testing import CliRunner

from boolsi_amd.cli import cli
from boolsi_amd.influence import InfluenceUsageError, average_sensitivity, build_sources, matrix_rows, summary_rows


@pytest.fixture
def model(tmp_path):
    path = tmp_path / 'net.yaml'
    path.write_text('nodes: [A, B, C, D]\nupdate rules: {A: B, B: A, C: A and D, D: C}\n'
                    'initial state: {A: any, B: any, C: 0, D: 1}\nfixed nodes: {D: 1}\n')
    return str(path)


@pytest.mark.parametrize('args,words', [
    (['-t', '3'], ['influence needs --samples']),
    (['-t', '3', '--seed', '1'], ['--seed needs --samples']),
    (['--samples', '8'], ['-t']),
    (['--samples', '8', '-t', '0'], ['-t']),
    (['--samples', '0', '-t', '3'], ['--samples']),
    (['--samples', '8', '-t', '3', '--nodes', 'A,X'], ["Unknown node 'X'"]),
    (['--samples', '8', '-t', '3', '--nodes', 'D'], ["'D'", 'fixed']),
    (['--samples', '8', '-t', '3', '--nodes', 'A,B,A'], ["'A'", 'twice']),
])
def test_usage_errors(model, tmp_path, args, words):
    res = CliRunner().invoke(cli, ['influence', model] + args + ['-o', str(tmp_path / 'out')])
    assert res.exit_code == 2, res.output
    assert 'Usage:' in res.output and all(w in res.output for w in words), res.output
    assert not (tmp_path / 'out').exists()


def test_the_command_is_documented():
    res = CliRunner().invoke(cli, ['influence', '--help'])
    assert res.exit_code == 0
    text = ' '.join(res.output.split())
    for option in ('--samples', '--seed', '--nodes', '-t', '-o'):
        assert option in text


NAMES = ['A', 'B', 'C', 'D', 'E']


def test_sources_come_in_node_order():
    assert build_sources(NAMES, {1: True, 3: False}) == [0, 2, 4]
    assert build_sources(NAMES, {}, ['E', 'B', 'C']) == [1, 2, 4]
    assert build_sources(NAMES, {0: True}, ['D']) == [3]
    for names, word in ((['A', 'Q'], 'Unknown'), (['B'], 'fixed'), (['C', 'C'], 'twice')):
        with pytest.raises(InfluenceUsageError, match=word):
            build_sources(NAMES, {1: True}, names)
    with pytest.raises(InfluenceUsageError, match='no source'):
        build_sources(['A', 'B'], {0: True, 1: False})


def test_rows_of_the_two_files():
    """2 sources, 2 steps, 5 nodes, 8 samples"""
    table = np.zeros((2, 2, 5), np.uint32)
    table[0, 0] = [0, 8, 0, 3, 0]
    table[0, 1, 4] = 5
    table[1, 0, 0] = 1
    merged = np.array([[0, 3], [7, 8]], np.uint64)
    assert matrix_rows(table, [1, 4], NAMES, 8) == [
        ['B', 1, 'B', 8, '1.0'], ['B', 1, 'D', 3, '0.375'], ['B', 2, 'E', 5, '0.625'], ['E', 1, 'A', 1, '0.125']]
    assert summary_rows(table, merged, [1, 4], NAMES, 8) == [
        ['B', 1, 8, '1.375', '0.0', 2], ['B', 2, 8, '0.625', '0.375', 1], ['E', 1, 8, '0.125', '0.875', 1], ['E', 2, 8, '0.0', '1.0', 0]]
    assert average_sensitivity(table, 8) == (11 + 1) / 16
    # the sums are taken in Python ints: counts near 2^32 do not wrap
    big = np.full((1, 1, 5), 2 ** 31, np.uint32)
    assert summary_rows(big, np.zeros((1, 1), np.uint64), [0], NAMES, 2 ** 31)[0][3] == '5.0'
    assert average_sensitivity(big, 2 ** 31) == 5.0
