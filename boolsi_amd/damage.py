"""
`damage` command: damage spreading over sampled pairs of states (Derrida curves).  For every requested number of
flips h, Engine.damage_sampled (bsx_run_damage_sampled, include/bsx.h has the definition) returns the sums over the
samples of the Hamming distance d(t) between a sampled state's trajectory and that of the same state with h free nodes
inverted; this module turns the integers into the rows of damage_spreading.csv and damage_histogram.csv.
"""
import csv
import logging
import math
import os

from .compile import compile_network, compile_space
from .output import list_texts


def parse_flips(text):
    """'1,2,4' -> [1, 2, 4]; ValueError for anything but positive integers."""
    flips = [int(part) for part in text.split(',')]
    if not flips or any(h < 1 for h in flips):
        raise ValueError(text)
    return flips


def damage_master(engine, origin_simulation_problem, simulation_problem_variations, predecessor_node_lists, truth_tables,
                  samples, seed, n_steps, flips, hist=False):
    """-> [(h, sum_d, sum_d2, n_merged, hist or None)] over samples 0 .. samples - 1 of `seed`, arrays of Python-int-able
    uint64, one entry per t = 0 .. n_steps."""
    log = logging.getLogger()
    net = compile_network(predecessor_node_lists, truth_tables)
    space = compile_space(origin_simulation_problem, simulation_problem_variations)
    engine.set_problem(net, space)
    log.info('Spreading damage over {} sampled pairs of states with seed {}, {} steps.'.format(samples, seed, n_steps))
    results, steps, ms = [], 0, 0.0
    for h in flips:
        sum_d, sum_d2, merged, cells, stats = engine.damage_sampled(seed, 0, samples, h, n_steps, hist=hist)
        results.append((h, sum_d, sum_d2, merged, cells))
        steps += stats['executed_steps']
        ms += stats['kernel_ms']
    log.info('Engine: {} state-steps in {:.1f} ms of kernels.'.format(steps, ms))
    return results


def curve_rows(results, samples, n_nodes):
    """Rows of damage_spreading.csv: flips, t, samples, mean_distance, normalized_distance, std_distance, merged_fraction.
    Floats as repr; the radicand of the standard deviation is taken in Python ints."""
    rows = []
    for h, sum_d, sum_d2, merged, _ in results:
        for t in range(len(sum_d)):
            s, s2, m = int(sum_d[t]), int(sum_d2[t]), int(merged[t])
            mean = s / samples
            rows.append([h, t, samples, repr(mean), repr(mean / n_nodes),
                         repr(math.sqrt(max(0, samples * s2 - s * s)) / samples), repr(m / samples)])
    return rows


def histogram_rows(results):
    """The nonzero (flips, t, distance, count) rows of damage_histogram.csv."""
    rows = []
    for h, _, _, _, cells in results:
        for t in range(len(cells)):
            rows.extend([h, t, k, int(cells[t][k])] for k in range(len(cells[t])) if cells[t][k])
    return rows


def output_damage(results, samples, n_nodes, output_dirpath, hist=False):
    os.makedirs(output_dirpath, exist_ok=True)
    files = ['"damage_spreading.csv"'] + (['"damage_histogram.csv"'] if hist else [])
    logging.getLogger().info('Printing damage spreading to {}...'.format(list_texts(files)))
    with open(os.path.join(output_dirpath, 'damage_spreading.csv'), 'w', newline='', encoding='utf-8') as f:
        writer = csv.writer(f)
        writer.writerow(['flips', 't', 'samples', 'mean_distance', 'normalized_distance', 'std_distance', 'merged_fraction'])
        writer.writerows(curve_rows(results, samples, n_nodes))
    if hist:
        with open(os.path.join(output_dirpath, 'damage_histogram.csv'), 'w', newline='', encoding='utf-8') as f:
            writer = csv.writer(f)
            writer.writerow(['flips', 't', 'distance', 'count'])
            writer.writerows(histogram_rows(results))
