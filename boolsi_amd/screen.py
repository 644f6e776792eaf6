"""
`screen` command: in-silico knockout / overexpression screens over sampled initial conditions.  Every mutant holds its
nodes at 0 or at 1 from t = 1 on and runs on the wild type's own samples (common random numbers), all of them in one
Engine.screen_sampled call (bsx_run_screen_sampled, include/bsx.h has the definition).  This module builds the mutant
list, and turns the integers that come back into the rows of screen_attractors.csv and screen_summary.csv.

Mutant order: the wild type; then every listed node in node order with its values in the order given; then, with pairs,
every pair i < j of the listed nodes with (v_i, v_j) in lexicographic order.
"""
import csv
import itertools
import logging
import os

from . import _lib
from .attract import merge_tables
from .compile import compile_network, compile_space
from .output import list_texts


class ScreenUsageError(ValueError):
    """A mutant list that cannot be built: the text is for the user."""


def parse_values(text):
    """'0,1' -> [0, 1]; ValueError for anything but a non-empty list of distinct 0 / 1."""
    values = [int(part) for part in text.split(',')]
    if not values or any(v not in (0, 1) for v in values) or len(set(values)) != len(values):
        raise ValueError(text)
    return values


def count_mutants(n_listed, n_values, pairs):
    return 1 + n_listed * n_values + (n_listed * (n_listed - 1) // 2 * n_values * n_values if pairs else 0)


def build_mutants(node_names, fixed_nodes, names=None, values=(0, 1), pairs=False):
    """-> list of mutants, each a tuple of (node index, value) pairs, in the order of the module's documentation.
    names: node names to screen (None: every node the origin does not fix); fixed_nodes: the origin's {node index: state}.
    ScreenUsageError for an unknown, repeated or origin-fixed name, and for more than BSX_SCREEN_MAX_MUTANTS mutants."""
    if names is None:
        listed = [i for i in range(len(node_names)) if i not in fixed_nodes]
    else:
        listed = []
        for name in names:
            if name not in node_names:
                raise ScreenUsageError("Unknown node '{}'.".format(name))
            node = node_names.index(name)
            if node in fixed_nodes:
                raise ScreenUsageError("Node '{}' is fixed by the input's 'fixed nodes' and cannot be screened.".format(name))
            if node in listed:
                raise ScreenUsageError("Node '{}' is listed twice.".format(name))
            listed.append(node)
        listed.sort()
    values = list(values)
    total = count_mutants(len(listed), len(values), pairs)
    if total > _lib.SCREEN_MAX_MUTANTS:
        raise ScreenUsageError('{} mutants are more than the 2^20 of one screen; list fewer nodes with --nodes.'.format(total))
    mutants = [()]
    mutants += [((node, v),) for node in listed for v in values]
    if pairs:
        mutants += [((a, va), (b, vb)) for a, b in itertools.combinations(listed, 2)
                    for va in sorted(values) for vb in sorted(values)]
    return mutants


def mutant_text(mutant, node_names):
    return ';'.join('{}={}'.format(node_names[node], value) for node, value in mutant) if mutant else 'wild type'


def screen_master(engine, origin_simulation_problem, simulation_problem_variations, predecessor_node_lists, truth_tables,
                  samples, seed, mutants, max_t, max_len):
    """-> (tables, none): per mutant the dict key -> [length, count, sum_l, sum_l2] in Python ints, and the number of
    samples without an attractor, over samples 0 .. samples - 1 of `seed`."""
    log = logging.getLogger()
    net = compile_network(predecessor_node_lists, truth_tables)
    space = compile_space(origin_simulation_problem, simulation_problem_variations)
    engine.set_problem(net, space)
    log.info('Screening {} mutants over {} sampled initial conditions with seed {}.'.format(len(mutants), samples, seed))
    records, none, stats = engine.screen_sampled(seed, 0, samples, mutants, max_t, max_len)
    log.info('Engine: {} state-steps in {:.1f} ms of kernels, {} host wait(s).'.format(
        stats['executed_steps'], stats['kernel_ms'], stats['host_syncs']))
    return [merge_tables([r]) for r in records], [int(x) for x in none]


def key_order(key):
    """The order of the engine's records: by the 64-bit words of the key state, from word 0."""
    return [(key >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(_lib.MAX_STATE_WORDS)]


def attractor_rows(tables, mutants, node_names, samples):
    """Rows of screen_attractors.csv: mutant, nodes, attractor (1-based, in the order of the engine's records), length,
    samples, frequency, mean_l, key (the key state as a 0/1 string in node order)."""
    n = len(node_names)
    rows = []
    for m, (table, mutant) in enumerate(zip(tables, mutants)):
        for i, (key, (length, count, sum_l, _)) in enumerate(sorted(table.items(), key=lambda item: key_order(item[0]))):
            rows.append([m, mutant_text(mutant, node_names), i + 1, length, count, repr(count / samples), repr(sum_l / count),
                         ''.join(str((key >> node) & 1) for node in range(n))])
    return rows


def moved_samples(wild, wild_none, table, none):
    """sum over the wild type's keys and the no-attractor bucket of max(0, c_wt - c_m): samples times the total-variation
    distance between the two distributions."""
    return sum(max(0, e[1] - table.get(key, (0, 0))[1]) for key, e in wild.items()) + max(0, wild_none - none)


def summary_rows(tables, none, mutants, node_names):
    """Rows of screen_summary.csv: mutant, nodes, attractors, fixed_points, samples_without_attractor, largest_basin,
    samples_in_wild_type_attractors, moved_samples."""
    wild, wild_none = tables[0], none[0]
    rows = []
    for m, (table, mutant) in enumerate(zip(tables, mutants)):
        rows.append([m, mutant_text(mutant, node_names), len(table), sum(1 for e in table.values() if e[0] == 1), none[m],
                     max((e[1] for e in table.values()), default=0), sum(e[1] for key, e in table.items() if key in wild),
                     moved_samples(wild, wild_none, table, none[m])])
    return rows


def output_screen(tables, none, mutants, node_names, samples, output_dirpath):
    os.makedirs(output_dirpath, exist_ok=True)
    logging.getLogger().info('Printing the screen to {}...'.format(list_texts(['"screen_attractors.csv"', '"screen_summary.csv"'])))
    with open(os.path.join(output_dirpath, 'screen_attractors.csv'), 'w', newline='', encoding='utf-8') as f:
        writer = csv.writer(f)
        writer.writerow(['mutant', 'nodes', 'attractor', 'length', 'samples', 'frequency', 'mean_l', 'key'])
        writer.writerows(attractor_rows(tables, mutants, node_names, samples))
    with open(os.path.join(output_dirpath, 'screen_summary.csv'), 'w', newline='', encoding='utf-8') as f:
        writer = csv.writer(f)
        writer.writerow(['mutant', 'nodes', 'attractors', 'fixed_points', 'samples_without_attractor', 'largest_basin',
                         'samples_in_wild_type_attractors', 'moved_samples'])
        writer.writerows(summary_rows(tables, none, mutants, node_names))
