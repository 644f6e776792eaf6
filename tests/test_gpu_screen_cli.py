"""
`screen FILE --samples N --seed S --nodes .. [--values ..] [--pairs]` end to end through the CLI: both CSVs equal, byte for
byte, text built here from the integers of the reference (screen_ref.ScreenRef over samples 0 .. N - 1) by the formulas of
the command's documentation.
"""
import faulthandler

import pytest

from boolsi_amd import synth

import sample_ref
from screen_ref import CASES, SEED, ScreenRef, compiled, moved_samples
from test_gpu_cli import read, run_cli
from wide_ref import aggregate

pytestmark = pytest.mark.gpu
N = 300
M64 = (1 << 64) - 1
# name -> (listed nodes, values, pairs, extra options)
RUNS = {
    'n300': ([299, 0], [0, 1], True, []),
    'n64': ([0, 2, 63], [1], False, ['-t', '40', '-a', '3']),
}


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def mutants_of_run(name):
    nodes, values, pairs, _ = RUNS[name]
    nodes = sorted(nodes)
    out = [()] + [((v, c),) for v in nodes for c in values]
    if pairs:
        out += [((a, ca), (b, cb)) for i, a in enumerate(nodes) for b in nodes[i + 1:] for ca in sorted(values) for cb in sorted(values)]
    return out


def reference_texts(name):
    net, space, _ = compiled(name)
    n = net.n_nodes
    options = RUNS[name][3]
    max_t = int(options[options.index('-t') + 1]) if '-t' in options else None
    max_len = int(options[options.index('-a') + 1]) if '-a' in options else None
    idx = sample_ref.sample_indices(space, SEED, range(N))
    mutants = mutants_of_run(name)
    results = [aggregate(ScreenRef(net, space, m).attract(idx, max_t, max_len)[0]) for m in mutants]
    wild, wild_none = results[0]
    attractors = ['mutant,nodes,attractor,length,samples,frequency,mean_l,key']
    summary = ['mutant,nodes,attractors,fixed_points,samples_without_attractor,largest_basin,samples_in_wild_type_attractors,moved_samples']
    for m, (mutant, (table, none)) in enumerate(zip(mutants, results)):
        text = ';'.join('{}={}'.format(synth.node_name(v), c) for v, c in mutant) if mutant else 'wild type'
        by_words = sorted(table, key=lambda key: [(key >> (64 * w)) & M64 for w in range(16)])
        for i, key in enumerate(by_words):
            length, count, sum_l, _ = table[key]
            attractors.append('{},{},{},{},{},{},{},{}'.format(m, text, i + 1, length, count, repr(count / N), repr(sum_l / count),
                                                               ''.join(str((key >> v) & 1) for v in range(n))))
        summary.append('{},{},{},{},{},{},{},{}'.format(
            m, text, len(table), sum(1 for e in table.values() if e[0] == 1), none, max((e[1] for e in table.values()), default=0),
            sum(e[1] for key, e in table.items() if key in wild), moved_samples(wild, wild_none, table, none)))
    # not vacuous: mutants that move samples, and (n64, under -t / -a) samples without an attractor
    assert any(r != results[0] for r in results[1:])
    if options:
        assert any(none for _, none in results)
    return ('\r\n'.join(attractors) + '\r\n').encode(), ('\r\n'.join(summary) + '\r\n').encode()


@pytest.mark.parametrize('name', list(RUNS))
def test_screen_cli_writes_the_reference_tables(tmp_path, name):
    (tmp_path / 'net.yaml').write_text(CASES[name]())
    nodes, values, pairs, options = RUNS[name]
    args = ['screen', str(tmp_path / 'net.yaml'), '--samples', str(N), '--seed', str(SEED), '--nodes', ','.join(synth.node_name(v) for v in nodes),
            '--values', ','.join(str(c) for c in values)] + (['--pairs'] if pairs else []) + options
    attractors, summary = reference_texts(name)
    out = run_cli(args, str(tmp_path / 'out'))
    assert 'Screening {} mutants over {} sampled initial conditions with seed {}'.format(len(mutants_of_run(name)), N, SEED) in out
    assert read(tmp_path / 'out' / 'screen_attractors.csv') == attractors
    assert read(tmp_path / 'out' / 'screen_summary.csv') == summary


def test_an_engine_error_is_logged_and_nothing_is_written(tmp_path):
    """An origin with a perturbation schedule: the CLI's policy for engine errors."""
    from sampled_cases import any_case
    (tmp_path / 'net.yaml').write_text(any_case(300, 2, 2, range(0, 40), perturbations={10: {'1': '2'}}))
    out = run_cli(['screen', str(tmp_path / 'net.yaml'), '--samples', '10', '--nodes', synth.node_name(0)], str(tmp_path / 'out'))
    assert 'Exception caught' in out and 'schedule' in out
    assert not (tmp_path / 'out' / 'screen_summary.csv').exists()
