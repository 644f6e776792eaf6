"""
Option checks of `target --samples` / `simulate --samples` that need no GPU: they are usage errors, raised before any
input is read or an engine opened (click's runner).
"""
import pytest
from click.testing import CliRunner

from boolsi_amd.cli import cli


@pytest.fixture
def model(tmp_path):
    path = tmp_path / 'net.yaml'
    path.write_text('nodes: [A, B]\nupdate rules: {A: B, B: A}\ninitial state: {A: any, B: any}\ntarget state: {A: 1}\n')
    return str(path)


@pytest.mark.parametrize('args', [['target', '--seed', '1'], ['simulate', '--seed', '1', '-t', '3']])
def test_seed_without_samples_is_a_usage_error(model, tmp_path, args):
    res = CliRunner().invoke(cli, [args[0], model] + args[1:] + ['-o', str(tmp_path / 'out')])
    assert res.exit_code == 2, res.output
    assert 'Usage:' in res.output and '--seed needs --samples' in res.output
    assert not (tmp_path / 'out').exists()


@pytest.mark.parametrize('args', [['target'], ['simulate', '-t', '3']])
def test_samples_with_a_reference_listing_is_a_usage_error(model, tmp_path, args):
    res = CliRunner().invoke(cli, [args[0], model] + args[1:] + ['--samples', '8', '--reference-np', '4', '-o', str(tmp_path / 'out')])
    assert res.exit_code == 2, res.output
    assert 'Usage:' in res.output and '--reference-np' in res.output and '--samples' in res.output
    assert not (tmp_path / 'out').exists()


@pytest.mark.parametrize('command', ['target', 'simulate', 'attract'])
def test_all_three_commands_take_the_same_seed_option(command):
    res = CliRunner().invoke(cli, [command, '--help'])
    assert res.exit_code == 0
    text = ' '.join(res.output.split())
    assert '--samples' in text and 'Seed of --samples: the same seed gives the same sample.' in text
