"""
`influence` command: the influence matrix I(v -> i, t) = P(node i differs at step t | node v was inverted at step 0) over
sampled initial conditions.  Every source node runs on the same samples, all of them in one Engine.influence_sampled call
(bsx_run_influence_sampled, include/bsx.h has the definition); this module builds the source list and turns the integers
that come back into the rows of influence_matrix.csv and influence_summary.csv.

Sources come in node order, whatever order --nodes names them in; the default is every node the origin does not fix.
"""
import csv
import logging
import os

from .compile import compile_network, compile_space
from .output import list_texts


class InfluenceUsageError(ValueError):
    """A source list that cannot be built: the text is for the user."""


def build_sources(node_names, fixed_nodes, names=None):
    """-> the source nodes in node order.  names: node names (None: every node the origin does not fix); fixed_nodes: the
    origin's {node index: state}.  InfluenceUsageError for an unknown, repeated or origin-fixed name, and for an empty list."""
    if names is None:
        listed = [i for i in range(len(node_names)) if i not in fixed_nodes]
    else:
        listed = []
        for name in names:
            if name not in node_names:
                raise InfluenceUsageError("Unknown node '{}'.".format(name))
            node = node_names.index(name)
            if node in fixed_nodes:
                raise InfluenceUsageError("Node '{}' is fixed by the input's 'fixed nodes' and cannot be a source.".format(name))
            if node in listed:
                raise InfluenceUsageError("Node '{}' is listed twice.".format(name))
            listed.append(node)
        listed.sort()
    if not listed:
        raise InfluenceUsageError("Every node is fixed by the input's 'fixed nodes': there is no source to invert.")
    return listed


def influence_master(engine, origin_simulation_problem, simulation_problem_variations, predecessor_node_lists, truth_tables,
                     samples, seed, n_steps, sources):
    """-> (influence uint32 (n_sources, n_steps, n), n_merged uint64 (n_sources, n_steps)) over samples 0 .. samples - 1 of
    `seed`."""
    log = logging.getLogger()
    net = compile_network(predecessor_node_lists, truth_tables)
    space = compile_space(origin_simulation_problem, simulation_problem_variations)
    engine.set_problem(net, space)
    log.info('Measuring the influence of {} nodes over {} sampled initial conditions with seed {}, {} steps.'.format(
        len(sources), samples, seed, n_steps))
    table, merged, stats = engine.influence_sampled(seed, 0, samples, sources, n_steps)
    log.info('Engine: {} state-steps in {:.1f} ms of kernels.'.format(stats['executed_steps'], stats['kernel_ms']))
    log.info('Average sensitivity of the network: {}.'.format(repr(average_sensitivity(table, samples))))
    return table, merged


def average_sensitivity(table, samples):
    """Sum over the sources of the t = 1 row sums / (samples * n_sources), the sums in Python ints."""
    return sum(int(v) for row in table[:, 0] for v in row) / (samples * len(table))


def matrix_rows(table, sources, node_names, samples):
    """Rows of influence_matrix.csv: source, t, target, count, probability -- the nonzero cells, by source, t and target."""
    rows = []
    for s, source in enumerate(sources):
        for t in range(table.shape[1]):
            cells = table[s, t]
            rows.extend([node_names[source], t + 1, node_names[i], int(cells[i]), repr(int(cells[i]) / samples)]
                        for i in cells.nonzero()[0].tolist())
    return rows


def summary_rows(table, merged, sources, node_names, samples):
    """Rows of influence_summary.csv: source, t, samples, mean_damage, merged_fraction, reach."""
    rows = []
    for s, source in enumerate(sources):
        for t in range(table.shape[1]):
            cells = table[s, t].tolist()
            rows.append([node_names[source], t + 1, samples, repr(sum(cells) / samples), repr(int(merged[s, t]) / samples),
                         sum(1 for v in cells if v)])
    return rows


def output_influence(table, merged, sources, node_names, samples, output_dirpath):
    os.makedirs(output_dirpath, exist_ok=True)
    logging.getLogger().info('Printing the influence matrix to {}...'.format(
        list_texts(['"influence_matrix.csv"', '"influence_summary.csv"'])))
    with open(os.path.join(output_dirpath, 'influence_matrix.csv'), 'w', newline='', encoding='utf-8') as f:
        writer = csv.writer(f)
        writer.writerow(['source', 't', 'target', 'count', 'probability'])
        writer.writerows(matrix_rows(table, sources, node_names, samples))
    with open(os.path.join(output_dirpath, 'influence_summary.csv'), 'w', newline='', encoding='utf-8') as f:
        writer = csv.writer(f)
        writer.writerow(['source', 't', 'samples', 'mean_damage', 'merged_fraction', 'reach'])
        writer.writerows(summary_rows(table, merged, sources, node_names, samples))
