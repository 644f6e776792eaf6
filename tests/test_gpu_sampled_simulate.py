"""
Simulate over sampled initial conditions (bsx_run_simulate_sampled, bsx_run_trajectories_sampled) against the exact
reference: sample_ref.sample_indices turns sample numbers into flat problem indices, WideRef.simulate / .trajectories runs
them.  Every comparison is exact equality on integers.
"""
import functools

import numpy as np
import pytest

from boolsi_amd import _lib

from sampled_cases import FIRST, L_OF, SEED, compiled
from sampled_target_cases import count_of, indices
from test_gpu_sampled import ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED, SCATTERED, engine
from test_gpu_wide_exact import words_array

pytestmark = pytest.mark.gpu
SIM_T = 40


@functools.lru_cache(maxsize=None)
def expect_simulate(name):
    net, space, ref = compiled(name)
    idx = indices(name, FIRST, count_of(name))
    traj, final, digest = ref.simulate(idx, SIM_T)
    assert len({tuple(t) for t in traj}) > len(traj) // 2 and len(set(final)) >= 2
    if name == 'n700_variations':
        assert len({ref.problem(i).tp for i in idx}) == 2 and len({i >> len(space.any_nodes) for i in idx}) >= 2
    return traj, final, digest


@pytest.mark.parametrize('name', ['n300', 'n1024', 'n700_variations'])
def test_simulate_sampled(monkeypatch, name):
    traj, final, digest = expect_simulate(name)
    net = compiled(name)[0]
    W, count = net.n_words, count_of(name)
    want = words_array(traj, W), words_array(final, W), np.array(digest, np.uint64)
    with engine(monkeypatch, name) as eng:
        assert eng.wide
        got = eng.simulate_sampled(SEED, FIRST, count, SIM_T)
        for g, w in zip(got[:3], want):
            assert np.array_equal(g, w)
        assert got[3]['problems'] == count and got[3]['state_steps'] == count * SIM_T
        # each sink alone
        for sink in range(3):
            flags = [sink == 0, sink == 1, sink == 2]
            alone = eng.simulate_sampled(SEED, FIRST, count, SIM_T, *flags)
            assert [a is not None for a in alone[:3]] == flags
            assert np.array_equal(alone[sink], want[sink])
            assert alone[3]['state_steps'] == count * SIM_T
        # additive over disjoint ranges
        cut = 100
        a = eng.simulate_sampled(SEED, FIRST, cut, SIM_T, trajectories=False)
        b = eng.simulate_sampled(SEED, FIRST + cut, count - cut, SIM_T, trajectories=False)
        assert np.array_equal(np.concatenate([a[2], b[2]]), want[2]) and np.array_equal(np.concatenate([a[1], b[1]]), want[1])


def test_simulate_sampled_refusals(monkeypatch):
    with engine(monkeypatch, 'n577') as eng:
        with pytest.raises(_lib.EngineError) as e:
            eng.simulate_sampled(SEED, 2 ** 64 - 10, 10, 4)
        assert e.value.status == ERR_INVALID
        with pytest.raises(_lib.EngineError) as e:
            eng.simulate_sampled(SEED, 0, 4, 1 << 30, trajectories=False)        # the step limit of bsx_run_simulate
        assert e.value.status == ERR_UNSUPPORTED
        last = eng.simulate_sampled(SEED, 2 ** 64 - 11, 10, 4, trajectories=False)
        ref = compiled('n577')[2]
        _, final, digest = ref.simulate(indices('n577', 2 ** 64 - 11, 10), 4)
        assert np.array_equal(last[1], words_array(final, 10)) and np.array_equal(last[2], np.array(digest, np.uint64))
        empty = eng.simulate_sampled(SEED, 5, 0, 4)
        assert empty[0].shape[0] == 0 and empty[3]['problems'] == 0
    with engine(monkeypatch) as eng:
        import ctypes as C
        st = _lib.Stats()
        assert eng._lib.bsx_run_simulate_sampled(eng._h, SEED, 0, 4, 4, None, None, None, C.byref(st)) == ERR_STATE
        assert eng._lib.bsx_run_trajectories_sampled(eng._h, SEED, None, None, 0, None, None, C.byref(st)) == ERR_STATE


# ---- trajectories of listed samples ----------------------------------------------------------------------------------

def listed(name):
    """At least G + 5 sample numbers: the scattered list of test_gpu_sampled.py (unsorted, across block boundaries, up to
    2^64 - 1), then seeded others; lengths 0 .. 12."""
    G = 32 * L_OF[name]
    rng = np.random.RandomState(len(name))
    more = [int(x) for x in rng.randint(0, 2 ** 62, G + 5 - len(SCATTERED), dtype=np.int64)]
    samples = SCATTERED + more
    t_len = [q % 13 for q in range(len(samples))]
    return samples, t_len


@functools.lru_cache(maxsize=None)
def expect_listed(name):
    net, space, ref = compiled(name)
    samples, t_len = listed(name)
    assert len(samples) >= 32 * L_OF[name] + 5 and samples != sorted(samples) and {0, 12} <= set(t_len)
    import sample_ref
    return ref.trajectories(sample_ref.sample_indices(space, SEED, samples), t_len)


@pytest.mark.parametrize('name', ['n1024', 'n700_variations', 'n64'])
def test_trajectories_sampled(monkeypatch, name):
    want = expect_listed(name)
    net = compiled(name)[0]
    W = net.n_words
    samples, t_len = listed(name)
    results = []
    for wide in ([False] if net.n_nodes > 256 else [False, True]):
        with engine(monkeypatch, name, wide=wide) as eng:
            assert eng.wide == (wide or net.n_nodes > 256)
            trajs, st = eng.trajectories_sampled(SEED, samples, t_len)
            assert st['problems'] == len(samples) and st['state_steps'] == sum(t_len)
            states, _ = eng.sample_problems(SEED, samples)
            for got, w, s0 in zip(trajs, want, states):
                assert np.array_equal(got, words_array(w, W)) and np.array_equal(got[0], s0)
            results.append(trajs)
            # non-contiguous places: every trajectory behind a gap of 3 words, the gaps keep their value
            sizes = [(t + 1) * W for t in t_len]
            offs = np.cumsum([3] + [s + 3 for s in sizes[:-1]]).astype(np.uint64)
            out = np.full(int(offs[-1]) + sizes[-1] + 3, 0x5A5A5A5A5A5A5A5A, np.uint64)
            import ctypes as C
            sm, tl = np.array(samples, np.uint64), np.array(t_len, np.uint64)
            stats = _lib.Stats()
            eng._check(eng._lib.bsx_run_trajectories_sampled(eng._h, SEED, _lib.ptr(sm), _lib.ptr(tl), len(sm), _lib.ptr(out), _lib.ptr(offs),
                                                             C.byref(stats)))
            covered = np.zeros(len(out), bool)
            for o, s, w in zip(offs.tolist(), sizes, want):
                assert np.array_equal(out[o:o + s].reshape(-1, W), words_array(w, W))
                covered[o:o + s] = True
            assert (out[~covered] == 0x5A5A5A5A5A5A5A5A).all() and (~covered).sum() == 3 * (len(samples) + 1)
    if len(results) == 2:           # the per-lane handle's second lowering and the wide handle agree
        assert all(np.array_equal(a, b) for a, b in zip(*results))
