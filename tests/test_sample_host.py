"""
boolsi_amd/csrc/bsx_sample.h without a GPU: the generator words A(b, a), the column words a sampled k_wide launch
stores into its bit-sliced matrix and the variant numbers, word for word against tests/sample_ref.py.
tests/sample_check.cpp is a stand-alone program that the host C++ compiler builds with no HIP include path, so it
compiles exactly the functions the kernels call; it is built a second time with the address and undefined-behaviour
sanitizers and run as its own process.

The sanity statistics of the definition follow: bit balance and the correlations between neighbours, as z-scores of
binomial counts (z = (ones - N / 2) / sqrt(N / 4) over N bits).  They are functions of the definition alone, so they
cannot flake; the bound is |z| <= 5 (a fair generator exceeds it with probability 6e-7 per statistic; this one stays
within 3.4).
"""
import functools
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import sample_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = {'plain': [], 'sanitized': ['-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']}

FIRSTS = [0, 1, 31, 33, 63, 64, 1000003]
N_ANYS = [1, 63, 64, 65, 300, 1024]
VS = [1, 2, 3, 6, 2 ** 63 + 5]
L = 8
COUNT = 32 * L + 37         # a whole group, then one with a full column, a column of 5 samples and six empty ones
SEED = 7


@pytest.fixture(scope='module')
def programs(tmp_path_factory):
    """kind -> the stand-alone program, built once per kind in pytest's own temporary directory."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    out = {}
    for kind, flags in FLAGS.items():
        out[kind] = str(tmp_path_factory.mktemp('sample_check') / ('sample_check_' + kind))
        subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror'] + flags +
                              ['-I' + os.path.join(ROOT, 'boolsi_amd', 'csrc'), os.path.join(ROOT, 'tests', 'sample_check.cpp'),
                               '-o', out[kind]])
    return out


def run(exe, *args):
    res = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    return [line.split() for line in res.stdout.splitlines()]


def sample_bits(seed, first, count, n_any):
    """uint64[count, n_any]: bit of 'any' ordinal a in sample first + q, from the words of the definition."""
    j = first + np.arange(count, dtype=np.uint64)
    b0 = first >> 6
    words = sample_ref.any_words_np(seed, ((first + count - 1) >> 6) - b0 + 1, n_any, b0)
    return (words[(j >> np.uint64(6)).astype(np.int64) - b0] >> (j & np.uint64(63))[:, None]) & np.uint64(1)


@pytest.mark.parametrize('kind', list(FLAGS))
def test_generator_words(programs, kind):
    for seed, b0 in itertools.product((0, 1, 7, 2 ** 63), (0, 4094, 2 ** 58 - 2)):
        lines = run(programs[kind], 'words', seed, b0, 2, 300)
        assert len(lines) == 600
        got = np.array([int(w, 16) for _, _, _, w in lines], np.uint64).reshape(2, 300)
        assert [int(b, 16) for _, b, _, _ in lines[::300]] == [b0, b0 + 1]
        assert np.array_equal(got, sample_ref.any_words_np(seed, 2, 300, b0))
        assert int(got[1, 299]) == sample_ref.any_word(seed, b0 + 1, 299)


@pytest.mark.parametrize('kind', list(FLAGS))
@pytest.mark.parametrize('n_any', N_ANYS)
def test_column_words_and_variants(programs, kind, n_any):
    for first, V in itertools.product(FIRSTS, VS):
        lines = run(programs[kind], 'columns', SEED, first, COUNT, n_any, V, L)
        bits = sample_bits(SEED, first, COUNT, n_any)
        want = np.zeros((2, L, n_any), np.uint64)           # [group][column][a]
        for q in range(COUNT):
            want[q // (32 * L), (q % (32 * L)) // 32] |= bits[q] << np.uint64(q % 32)
        cols = [l for l in lines if l[0] == 'C']
        assert len(cols) == 2 * L * n_any
        got = np.array([int(l[4], 16) for l in cols], np.uint64).reshape(2, L, n_any)
        assert np.array_equal(got, want)
        assert not want[1, 2:].any() and want[1, 1].max() < 32          # the ragged column and the empty ones
        variants = [(int(l[1], 16), int(l[2], 16)) for l in lines if l[0] == 'V']
        assert variants == [(q, (sample_ref.draw(SEED, first + q, n_any) * V) >> 64) for q in range(COUNT)]
        assert all(v < V for _, v in variants)
    # a column word spelled out bit by bit in Python ints, for one unaligned column that straddles two blocks
    assert int(want[0, 1, n_any - 1]) == sample_ref.column_word(SEED, FIRSTS[-1] + 32, n_any - 1, 32)


@pytest.mark.parametrize('kind', list(FLAGS))
def test_single_samples(programs, kind):
    samples = [0, 63, 64, 1000003, 2 ** 64 - 1]
    for n_any, V in ((1, 1), (65, 6), (1024, 2 ** 63 + 5)):
        lines = run(programs[kind], 'problems', SEED, n_any, V, *samples)
        for j, (_, js, variant, bits) in zip(samples, lines):
            want_bits, want_variant = sample_ref.sample(SEED, j, n_any, V)
            assert int(js, 16) == j and int(variant, 16) == want_variant
            assert [int(c) for c in bits] == want_bits


# ---- sanity statistics of the definition ----------------------------------------------------------------------------

N_BLOCKS, STAT_ANY = 4096, 300


def z_of(ones, n):
    return (float(ones) - n / 2) / (n / 4) ** 0.5


def ones_of(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


@functools.lru_cache(maxsize=None)
def stat_words(seed):
    return sample_ref.any_words_np(seed, N_BLOCKS, STAT_ANY)


@pytest.mark.parametrize('seed', [0, 1, 7, 2 ** 63])
def test_balance_and_neighbour_correlations(seed):
    A = stat_words(seed)
    n = A.size * 64
    z = {'balance': z_of(ones_of(A), n)}
    # agreement of neighbours = zeros of the xor, so z of the xor's ones is minus the correlation's z
    adj = A ^ (A >> np.uint64(1))
    z['adjacent samples'] = z_of(ones_of(adj & np.uint64((1 << 63) - 1)), A.size * 63)
    z['adjacent nodes'] = z_of(ones_of(A[:, 1:] ^ A[:, :-1]), A[:, 1:].size * 64)
    z['adjacent blocks'] = z_of(ones_of(A[1:] ^ A[:-1]), A[1:].size * 64)
    bits = np.unpackbits(np.ascontiguousarray(A).view(np.uint8).reshape(N_BLOCKS, STAT_ANY, 8), axis=2, bitorder='little')
    per_node = bits.sum(axis=(0, 2))
    z['per node'] = max(abs(z_of(c, N_BLOCKS * 64)) for c in per_node)
    per_lane = bits.reshape(N_BLOCKS, STAT_ANY, 64).sum(axis=(0, 1))
    z['per lane'] = max(abs(z_of(c, N_BLOCKS * STAT_ANY)) for c in per_lane)
    print(seed, z)
    assert all(abs(v) <= 5 for v in z.values()), z


def test_neighbouring_seeds_are_uncorrelated():
    x = stat_words(5) ^ stat_words(6)
    z = z_of(ones_of(x), x.size * 64)
    print(z)
    assert abs(z) <= 5
