"""
Target mode against the CPU oracle, exactly: the hit list of bsx_run_target (k_target, k_compact_count / k_compact_write)
and the count, histogram and listed hits of bsx_run_target_summary with and without cube passes, on the members of
tests/target_family.py (tests/test_target_family.py proves on the CPU that their targets are reached late, at the cap,
at t = 0 by part of a cube class, ...).  Every comparison is integer equality with Oracle.target or, for the chain
members, with the closed form.  The step statistic is not compared with the oracle (the kernel counts Brent's stop
time, the oracle mu + lambda), only list against summary under BSX_CUBES=0.
"""
from math import inf

import numpy as np
import pytest

from target_family import BY_NAME, FAMILY, N_FUZZ, fuzz_member

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from boolsi_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def set_member(eng, member, monkeypatch, lut_mode=None):
    _, _, net, space, mask, code = member.compiled()
    if lut_mode is not None:
        monkeypatch.setenv('BSX_LUT_MODE', lut_mode)
    eng.set_problem(net, space)
    monkeypatch.delenv('BSX_LUT_MODE', raising=False)
    return mask, code


def expected(member, first, count, max_t):
    """(offsets, first-hit times) of the reached problems, ascending"""
    return member.closed_form(first, count, max_t) if member.chain else member.reference(first, count, max_t)


def same_list(hits, off, t):
    assert np.array_equal(hits['offset'], off) and np.array_equal(hits['t'], t)


def histogram(t, bins):
    return np.bincount(np.minimum(t, np.uint64(bins - 1)).astype(np.int64), minlength=bins).tolist() if bins else []


def check_summaries(eng, first, count, max_t, mask, code, off, t, monkeypatch, caps, bins_list, steps=None):
    for cubes in (None, '0'):
        if cubes is None:
            monkeypatch.delenv('BSX_CUBES', raising=False)
        else:
            monkeypatch.setenv('BSX_CUBES', cubes)
        for cap in caps:
            for bins in bins_list:
                total, hist, listed, st = eng.target_summary(first, count, max_t, mask, code, hist_bins=bins, cap=cap)
                where = 'BSX_CUBES {}, cap {}, hist_bins {}'.format(cubes, cap, bins)
                assert total == len(off), where
                assert hist.tolist() == histogram(t, bins), where
                assert len(listed) == min(cap, len(off)), where
                same_list(listed, off[:cap], t[:cap])
                if cubes == '0' and steps is not None:
                    assert st['state_steps'] == steps, where
    monkeypatch.delenv('BSX_CUBES', raising=False)


CASES = [(mb, max_t, lm) for mb in FAMILY for max_t in mb.max_ts for lm in mb.lut_modes]


@pytest.mark.parametrize('member,max_t,lut_mode', CASES, ids=lambda v: 'lut' + v if isinstance(v, str) else str(v))
def test_list_and_summary_equal_the_oracle(eng, member, max_t, lut_mode, monkeypatch):
    mask, code = set_member(eng, member, monkeypatch, lut_mode)
    for first, count, _ in member.ranges:
        off, t = expected(member, first, count, max_t)
        hits, st = eng.target(first, count, max_t, mask, code)
        same_list(hits, off, t)
        tmax = int(t.max()) if len(t) else 0
        bins_list = [min(tmax + 2, 2048) if b is None else b for b in member.hist_bins]
        check_summaries(eng, first, count, max_t, mask, code, off, t, monkeypatch, (0, 5, len(off), len(off) + 3), bins_list,
                        steps=st['state_steps'])
        # partition invariance: three unequal pieces add up to the whole
        cuts = [0, count // 7, count // 7 + count // 2 + 1, count]
        bins = min(tmax + 2, 2048)
        total, hist = 0, np.zeros(bins, np.uint64)
        for a, b in zip(cuts, cuts[1:]):
            n, h, _, _ = eng.target_summary(first + a, b - a, max_t, mask, code, hist_bins=bins)
            total += n
            hist += h
        assert total == len(off) and hist.tolist() == histogram(t, bins)


@pytest.mark.parametrize('member', [mb for mb in FAMILY if mb.cubes_expected], ids=str)
def test_cube_passes_run_where_they_are_expected(eng, member, monkeypatch, capfd):
    """bsx_run_target_summary falls back to the plain pass in silence; its debug line is the only witness of a cube pass"""
    mask, code = set_member(eng, member, monkeypatch)
    monkeypatch.delenv('BSX_CUBES', raising=False)
    monkeypatch.setenv('BSX_DEBUG', '1')
    max_t = member.max_ts[0]
    for first, count, claims in member.ranges:
        off, t = expected(member, first, count, max_t)
        for cap in (0, 5) if 'block' in claims else (0,):
            if cap:         # the first listing piece is 2^16 problems long and must fill the list, an aligned block follows it
                assert int((off < 1 << 16).sum()) >= cap and count >= 1 << 17 and first % (1 << 16) == 0
            capfd.readouterr()
            total, _, listed, _ = eng.target_summary(first, count, max_t, mask, code, cap=cap)
            err = capfd.readouterr().err
            assert 'target cube' in err, (first, count, cap)
            assert total == len(off)
            same_list(listed, off[:cap], t[:cap])


def test_compaction_at_segment_edges(eng, monkeypatch):
    """Counts of 1, 4095, 4096, 4097 and 8193 problems with a hit in the last slot of a 4096-segment (and, where the
    range goes on, in its very last problem)."""
    member = BY_NAME['n20_k2']
    mask, code = set_member(eng, member, monkeypatch)
    off, _ = member.reference(0, 1 << 17, inf)
    is_hit = np.zeros(1 << 17, bool)
    is_hit[off.astype(np.int64)] = True
    for count in (1, 4095, 4096, 4097, 8193):
        slot = min(count, 4096) - 1
        first = next(int(h) - slot for h in off.tolist() if 8192 <= h < (1 << 16) and is_hit[int(h) - slot + count - 1])
        roff, rt = member.reference(first, count, inf)
        assert slot in roff.tolist() and count - 1 in roff.tolist()
        hits, _ = eng.target(first, count, inf, mask, code)
        same_list(hits, roff, rt)
        total, hist, listed, _ = eng.target_summary(first, count, inf, mask, code, hist_bins=3, cap=len(roff))
        assert total == len(roff) and hist.tolist() == histogram(rt, 3)
        same_list(listed, roff, rt)


def test_a_full_hit_table_is_an_error_and_the_handle_lives_on(eng, monkeypatch):
    from boolsi_amd._lib import ERR_TABLE_FULL, EngineError
    member = BY_NAME['n20_k2']
    mask, code = set_member(eng, member, monkeypatch)
    first, count, _ = member.ranges[1]
    off, t = member.reference(first, count, 6)
    assert ERR_TABLE_FULL == -5 and len(off) > 1
    with pytest.raises(EngineError) as e:
        eng.target(first, count, 6, mask, code, cap=len(off) - 1)
    assert e.value.status == -5
    hits, _ = eng.target(first, count, 6, mask, code, cap=len(off))
    same_list(hits, off, t)


@pytest.mark.parametrize('seed', range(N_FUZZ))
def test_random_networks_with_reached_targets(eng, seed, monkeypatch):
    member = fuzz_member(seed)
    mask, code = set_member(eng, member, monkeypatch)
    (first, count, _), = member.ranges
    max_t, = member.max_ts
    off, t = member.reference(first, count, max_t)
    hits, st = eng.target(first, count, max_t, mask, code)
    same_list(hits, off, t)
    check_summaries(eng, first, count, max_t, mask, code, off, t, monkeypatch, (0, 5), (0, 7, 66), steps=st['state_steps'])
