"""
`screen`: the option checks and the mutant order, which need no GPU.  Usage errors are raised before the output directory
is made or an engine opened (click's runner); the mutant order is that of boolsi_amd/screen.py: the wild type, every listed
node in node order with its values in the order given, then (--pairs) every pair i < j with the value pairs in
lexicographic order.
"""
import pytest
from click.testing import CliRunner

from boolsi_amd import _lib
from boolsi_amd.cli import cli
from boolsi_amd.screen import ScreenUsageError, build_mutants, count_mutants, mutant_text, parse_values


@pytest.fixture
def model(tmp_path):
    path = tmp_path / 'net.yaml'
    path.write_text('nodes: [A, B, C, D]\nupdate rules: {A: B, B: A, C: A and D, D: C}\n'
                    'initial state: {A: any, B: any, C: 0, D: 1}\nfixed nodes: {D: 1}\n')
    return str(path)


@pytest.mark.parametrize('args,words', [
    ([], ['screen needs --samples']),
    (['--seed', '1'], ['--seed needs --samples']),
    (['--samples', '8', '--nodes', 'A,X'], ["Unknown node 'X'"]),
    (['--samples', '8', '--nodes', 'D'], ["'D'", 'fixed']),
    (['--samples', '8', '--nodes', 'A,A'], ["'A'", 'twice']),
    (['--samples', '8', '--values', '0,2'], ['--values']),
    (['--samples', '8', '--values', '1,1'], ['--values']),
    (['--samples', '0'], ['--samples']),
])
def test_usage_errors(model, tmp_path, args, words):
    res = CliRunner().invoke(cli, ['screen', model] + args + ['-o', str(tmp_path / 'out')])
    assert res.exit_code == 2, res.output
    assert 'Usage:' in res.output and all(w in res.output for w in words), res.output
    assert not (tmp_path / 'out').exists()


def test_the_command_is_documented():
    res = CliRunner().invoke(cli, ['screen', '--help'])
    assert res.exit_code == 0
    text = ' '.join(res.output.split())
    for option in ('--samples', '--seed', '--nodes', '--values', '--pairs', '-t', '-a', '-o'):
        assert option in text


NAMES = ['A', 'B', 'C', 'D', 'E']


def test_the_default_list_is_every_node_the_origin_does_not_fix():
    got = build_mutants(NAMES, {1: True, 3: False})
    assert got == [(), ((0, 0),), ((0, 1),), ((2, 0),), ((2, 1),), ((4, 0),), ((4, 1),)]
    assert len(got) == count_mutants(3, 2, False)


def test_nodes_come_in_node_order_and_values_in_the_order_given():
    assert build_mutants(NAMES, {}, ['E', 'B'], [1, 0]) == [(), ((1, 1),), ((1, 0),), ((4, 1),), ((4, 0),)]
    assert build_mutants(NAMES, {}, ['C'], [1]) == [(), ((2, 1),)]


def test_pairs_follow_the_single_mutants():
    got = build_mutants(NAMES, {3: True}, ['E', 'A', 'C'], [0, 1], pairs=True)
    singles = [((0, 0),), ((0, 1),), ((2, 0),), ((2, 1),), ((4, 0),), ((4, 1),)]
    pairs = [((a, va), (b, vb)) for a, b in ((0, 2), (0, 4), (2, 4)) for va, vb in ((0, 0), (0, 1), (1, 0), (1, 1))]
    assert got == [()] + singles + pairs
    assert len(got) == count_mutants(3, 2, True) == 19
    # one value: one pair of values
    assert build_mutants(NAMES, {}, ['A', 'B'], [1], pairs=True) == [(), ((0, 1),), ((1, 1),), ((0, 1), (1, 1))]
    # the value pairs are in lexicographic order whatever order the values were given in
    assert build_mutants(NAMES, {}, ['A', 'B'], [1, 0], pairs=True)[5:] == [((0, va), (1, vb)) for va in (0, 1) for vb in (0, 1)]


def test_more_than_2_to_20_mutants_is_refused():
    names = ['n{}'.format(i) for i in range(1025)]
    assert count_mutants(1025, 2, True) > _lib.SCREEN_MAX_MUTANTS >= count_mutants(1025, 2, False)
    with pytest.raises(ScreenUsageError, match='2\\^20'):
        build_mutants(names, {}, None, [0, 1], pairs=True)
    assert len(build_mutants(names, {}, None, [0, 1])) == 2051


def test_texts_and_values():
    assert mutant_text((), NAMES) == 'wild type'
    assert mutant_text(((0, 0), (4, 1)), NAMES) == 'A=0;E=1'
    assert parse_values('0,1') == [0, 1] and parse_values('1') == [1]
    for bad in ('', '2', '0,0', 'x'):
        with pytest.raises(ValueError):
            parse_values(bad)
