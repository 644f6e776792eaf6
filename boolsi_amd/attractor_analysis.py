"""
Node correlations across attractors: frequency-weighted Spearman's rho and two-sided p-values
(reference `boolsi/attractor_analysis.py:29-145`; SURVEY f-3).

Two paths to rho: host-side numpy (ranks by one sort per node column, then np.cov), as the reference does it, for
small tables; and for tables of DEVICE_CORRELATION_CELLS cells or more one device call (Engine.node_correlations,
DESIGN.md "Node correlations") that returns S = sum_q f_q d2_qa d2_qb over exact centred integer ranks.  Both hand
their matrix to correlation_statistics(), which forms rho, t and the p-values.
"""
import logging
from math import inf

import numpy as np
from scipy import stats


def weighted_ranks(values, weights):
    """Average ranks of `values` when value i occurs weights[i] times."""
    order = np.argsort(values, kind='stable')
    sorted_values = values[order]
    uniq, start, inverse = np.unique(sorted_values, return_index=True, return_inverse=True)
    group_weight = np.add.reduceat(weights[order], start)
    before = np.concatenate(([0], np.cumsum(group_weight)[:-1]))
    group_rank = before + 0.5 * (group_weight + 1)
    ranks = np.empty(len(values), dtype=float)
    ranks[order] = group_rank[inverse]
    return ranks


# Tables of at least this many cells (attractors x nodes) take the device path when an engine is at hand.  Measured
# (tools/bench_correlations.py, profiles/node_correlations.json): every device run beats every host
# run from 2^12 cells up at 64 and at 1024 nodes, so the constant is the floor -- below it nothing is gained, and every
# published example stays on the host path, byte for byte.
DEVICE_CORRELATION_CELLS = 1 << 12


def correlation_statistics(cross, dof):
    """rho and two-sided t-test p-values from a matrix proportional to the covariance of the ranks (np.cov's, or the
    device's S: the scale cancels in rho).  A zero on the diagonal (a constant node) makes its pairs NaN."""
    var = cross.diagonal()
    with np.errstate(invalid='ignore', divide='ignore'):
        r = cross / np.sqrt(np.multiply.outer(var, var))
        t = r / np.sqrt((1 - r * r) / dof)
        p = 2 * stats.t.sf(np.abs(t), dof)
    return r, p


def weighted_pearson(data, weights):
    """Pearson r between columns of `data` with integer row weights, and t-test p-values."""
    return correlation_statistics(np.cov(data.T, fweights=weights), weights.sum() - 2)


def compute_frequency_spearmanrho(data, frequencies):
    ranks = np.column_stack([weighted_ranks(data[:, j], frequencies) for j in range(data.shape[1])])
    return weighted_pearson(ranks, frequencies)


def uses_device(n_attractors, n_nodes, engine=None, device=None):
    """Which path find_node_correlations takes: `device` True / False forces one (tests, A/B runs); None applies the
    size rule, and without an engine there is only the host path."""
    if device is not None:
        return bool(device)
    return engine is not None and n_attractors * n_nodes >= DEVICE_CORRELATION_CELLS


def find_node_correlations(attractors, engine=None, device=None):
    """attractors: list of AggregatedAttractor with .frequency and .activity or .states -> (Rho, P) or None.
    An observation is a node's mean state over the attractor: .activity (on-counts / length, from the device) where it
    is there, else the mean over .states -- the same float64, an exact integer sum divided by the length.
    With an `engine` (its problem set, as attract_master leaves it) large tables go through one device call that needs
    only key, length and frequency of every attractor (uses_device); a table the device call refuses for its size
    (total frequency of 2^62 or more, more than 2^31 cells) takes the host path."""
    log = logging.getLogger()
    total = sum(a.frequency for a in attractors)
    if len(attractors) == 1 or total <= 2:
        log.info('Not enough attractors to infer node correlations.')
        return None
    if engine is not None and uses_device(len(attractors), engine.net.n_nodes, engine, device):
        from ._lib import EngineError, ERR_RANGE_TOO_LARGE, ERR_UNSUPPORTED
        log.info('Computing node correlations on the device ({} attractors x {} nodes)...'.format(
            len(attractors), engine.net.n_nodes))
        try:
            S, _, _, closed = engine.node_correlations([a.key for a in attractors], [a.length for a in attractors],
                                                       [a.frequency for a in attractors])
        except EngineError as e:
            if e.status not in (ERR_RANGE_TOO_LARGE, ERR_UNSUPPORTED):
                raise
            log.info('The device call does not take this table ({}); computing node correlations on the host.'.format(e))
        else:
            for a, c in zip(attractors, closed):
                if not c:
                    raise RuntimeError('attractor {} does not return to its key state after {} steps'.format(a.key, a.length))
            return correlation_statistics(S, total - 2)
    elif device:
        raise ValueError('the device path needs an engine')
    if engine is not None and any(getattr(a, 'activity', None) is None and a.states is None for a in attractors):
        from .attract import profile_attractors
        profile_attractors(engine, attractors, with_states=False, with_activity=True)
    observations = np.array([a.activity if getattr(a, 'activity', None) is not None else
                             np.mean(np.array(a.states, dtype=float), axis=0) for a in attractors])
    frequencies = np.array([a.frequency for a in attractors])
    log.info('Computing node correlations...')
    return compute_frequency_spearmanrho(observations, frequencies)


def attractor_transitions(engine, attractors, max_t=inf):
    """
    Stability of the attractors of a finished table under a single flip of one node (Engine.attractor_transitions): for
    every attractor, every one of its states and every node that the origin problem does not fix, the node is flipped
    once and the network followed until it is on a cycle again.
    -> (edges, n_free): the engine's edge records (src and dst index `attractors`; dst may be _lib.TRANS_OUTSIDE or
    _lib.TRANS_UNRESOLVED) and the number of free nodes, so that attractor q has length_q * n_free flips.
    Networks on the wide-state family go through Engine.attractor_transitions_wide.
    """
    call = engine.attractor_transitions_wide if engine.wide else engine.attractor_transitions
    edges, _, closed = call([a.key for a in attractors], [a.length for a in attractors], max_t=max_t,
                            edge_cap=max(1, min(1 << 24, len(attractors) * (len(attractors) + 2))))
    for a, ok in zip(attractors, closed):
        if not ok:
            raise RuntimeError('attractor {} does not return to its key state after {} steps'.format(a.key, a.length))
    n_free = engine.net.n_nodes - len({int(node) for node in engine.space.fixed[:, 0]})
    return edges, n_free
