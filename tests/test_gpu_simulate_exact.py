"""
Simulate mode against the CPU oracle, exactly: final states, digests and whole trajectories of bsx_run_simulate on its
three kernels (k_simulate, k_simulate_sliced, k_simulate_sliced64), the router's thresholds and shape rules, the second
pass of each kernel's outer loop, and bsx_run_trajectories with scattered lists, on the members of
tests/simulate_family.py (tests/test_simulate_family.py proves on the CPU that no member is vacuous).  Every comparison is
integer equality with Oracle.simulate or Oracle.trajectory; the route a call took is read from its BSX_DEBUG line.
"""
import ctypes as C
import re
from math import inf

import numpy as np
import pytest

from simulate_family import BY_NAME, FAMILY, PER_LANE, SECOND_PASS, SLICED, SLICED64, TRAJ_MEMBERS, CORES

pytestmark = pytest.mark.gpu

LINE = re.compile(r'\[bsx\] simulate: (per-lane|sliced64|sliced), (\d+) blocks(?:, (\d+) groups)?')
GROUP = {SLICED: 2048, SLICED64: 4096}


@pytest.fixture(scope='module')
def eng():
    from boolsi_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def set_problem(eng, net, space, monkeypatch, lut_mode=None):
    if lut_mode is not None:
        monkeypatch.setenv('BSX_LUT_MODE', lut_mode)
    eng.set_problem(net, space)
    monkeypatch.delenv('BSX_LUT_MODE', raising=False)
    monkeypatch.setenv('BSX_DEBUG', '1')


def knob(monkeypatch, value):
    if value is None:
        monkeypatch.delenv('BSX_SLICED', raising=False)
    else:
        monkeypatch.setenv('BSX_SLICED', value)


def run(eng, capfd, first, count, max_t, trajectories=False, final=True, digest=False):
    """-> (trajectories, final states, digests, stats, (route, blocks, groups)) of one bsx_run_simulate call"""
    capfd.readouterr()
    traj, fin, dig, st = eng.simulate(first, count, max_t, trajectories=trajectories, final=final, digest=digest)
    lines = LINE.findall(capfd.readouterr().err)
    assert len(lines) == 1, lines
    route, blocks, groups = lines[0]
    assert st['state_steps'] == count * max_t and st['problems'] == count
    return traj, fin, dig, st, (route, int(blocks), int(groups) if groups else None)


CASES = [(mb, max_t, lm) for mb in FAMILY for max_t in mb.max_ts for lm in mb.lut_modes]


@pytest.mark.parametrize('member,max_t,lut_mode', CASES, ids=lambda v: 'lut' + v if isinstance(v, str) else str(v))
def test_every_sink_on_every_route_equals_the_oracle(eng, member, max_t, lut_mode, monkeypatch, capfd):
    set_problem(eng, *member.compiled(), monkeypatch, lut_mode)
    for r in member.ranges:
        ofin, odig = member.reference(r.first, r.count, max_t)
        if r.route == PER_LANE:
            knob(monkeypatch, None)
            traj, fin, dig, _, (route, blocks, _) = run(eng, capfd, r.first, r.count, max_t, trajectories=True, digest=True)
            assert route == PER_LANE and blocks == (r.count + 511) // 512
            assert np.array_equal(traj, member.trajectories(r.first, r.count, max_t))
            assert np.array_equal(fin, ofin) and np.array_equal(dig, odig)
            _, fin, dig, _, _ = run(eng, capfd, r.first, r.count, max_t, final=False, digest=True)
            assert fin is None and np.array_equal(dig, odig)
            _, fin, _, _, _ = run(eng, capfd, r.first, r.count, max_t)
            assert np.array_equal(fin, ofin)
            continue
        for value in (None, '0', '1'):
            knob(monkeypatch, value)
            for final, digest in ((True, False), (True, True), (False, True)):
                _, fin, dig, _, (route, blocks, groups) = run(eng, capfd, r.first, r.count, max_t, final=final, digest=digest)
                where = 'BSX_SLICED {}, final {}, digest {}'.format(value, final, digest)
                assert route == member.route(r, digest=digest, knob=value), where
                if route != PER_LANE:
                    assert groups == (r.count + GROUP[route] - 1) // GROUP[route] == blocks, where
                assert not final or np.array_equal(fin, ofin), where
                assert not digest or np.array_equal(dig, odig), where
    knob(monkeypatch, None)


@pytest.mark.parametrize('name', ['g2_n17_k2', 'g1_k4_n17'])
def test_both_sides_of_the_routers_thresholds(eng, name, monkeypatch, capfd):
    member = BY_NAME[name]
    set_problem(eng, *member.compiled(), monkeypatch)
    knob(monkeypatch, None)
    (r,) = member.ranges
    for count in (2047, 2048, 2049):
        for max_t in (63, 64, 65):
            ofin, _ = member.reference(r.first, count, max_t)
            _, fin, _, _, (route, _, _) = run(eng, capfd, r.first, count, max_t)
            assert route == (r.route if count >= 2048 and max_t >= 64 else PER_LANE), (count, max_t)
            assert np.array_equal(fin, ofin), (count, max_t)


@pytest.mark.parametrize('name,first,count,digest', [
    ('g1_k4_n17', None, 2048 + 37, True),           # digests: the second-generation kernel alone has them, K <= 3 ...
    ('g1_k2_n129', None, 2048 + 37, True),          # ... and at most 128 rows
    ('var_n40', 512 * 24 - 2000, 4096 + 37, False),  # variations
    ('mixed9_n40', None, 2048 + 37, False),         # a wide rule
])
def test_shapes_the_sliced_kernels_do_not_take_go_per_lane(eng, name, first, count, digest, monkeypatch, capfd):
    member = BY_NAME[name]
    set_problem(eng, *member.compiled(), monkeypatch)
    knob(monkeypatch, None)
    first = member.ranges[0].first if first is None else first
    ofin, odig = member.reference(first, count, 64)
    _, fin, dig, _, (route, _, _) = run(eng, capfd, first, count, 64, digest=digest)
    assert route == PER_LANE
    assert np.array_equal(fin, ofin) and (not digest or np.array_equal(dig, odig))


# ---- second passes of the three outer loops --------------------------------------------------------------------------

def load(eng, text, monkeypatch):
    from boolsi_amd.compile import compile_problem
    from boolsi_amd.constants import Mode
    from boolsi_amd.input import parse_input_text
    from oracle.cpu_oracle import Oracle
    net, space = compile_problem(parse_input_text(text, inf, Mode.SIMULATE))
    set_problem(eng, net, space, monkeypatch)
    return net, space, Oracle(net, space)


@pytest.mark.parametrize('kind,first,per_cu', [(SLICED, (1 << 129) + (1 << 65) + 77, 2), (SLICED64, 77, 1)])
def test_second_pass_of_a_sliced_group_loop(eng, kind, first, per_cu, monkeypatch, capfd):
    """More groups than workgroups: a workgroup re-initialises its rows and runs a second group."""
    net, space, orc = load(eng, SECOND_PASS[kind], monkeypatch)
    if kind == SLICED:
        rows = (net.n_nodes + 15) & ~15
        assert (160 * 1024) // (rows * 136 * 4) == per_cu           # workgroups of this shape that share a CU's LDS
    cus = eng.device_info()['compute_units']
    group, max_t = GROUP[kind], 64
    count = cus * per_cu * group + group + 37
    assert first + count <= space.n_problems
    knob(monkeypatch, None)
    _, fin, _, _, (route, blocks, groups) = run(eng, capfd, first, count, max_t)
    assert route == kind and blocks == cus * per_cu and groups == blocks + 2 > blocks
    knob(monkeypatch, '0')
    _, lane, _, _, (route, _, _) = run(eng, capfd, first, count, max_t)
    knob(monkeypatch, None)
    assert route == PER_LANE and np.array_equal(fin, lane)
    # the oracle on the start, on the first group of the second pass and on the ragged end
    for at, length in ((0, 2048), (blocks * group, 2048), (count - 2048 - 37, 2048 + 37)):
        ofin = orc.simulate(first + at, length, max_t, want_traj=False, n_threads=CORES)[1]
        assert np.array_equal(fin[at:at + length], ofin), at


def test_second_pass_of_the_per_lane_grid_stride_loop(eng, monkeypatch, capfd):
    net, space, orc = load(eng, SECOND_PASS[PER_LANE], monkeypatch)
    cus = eng.device_info()['compute_units']
    first, max_t, count = 77, 4, 4 * cus * 512 + 512 + 37
    assert first + count <= space.n_problems
    _, fin, dig, _, (route, blocks, _) = run(eng, capfd, first, count, max_t, digest=True)
    assert route == PER_LANE and blocks == 4 * cus and count > blocks * 512
    _, ofin, odig, _ = orc.simulate(first, count, max_t, want_traj=False, n_threads=CORES)
    assert np.array_equal(fin, ofin) and np.array_equal(dig, odig)


# ---- bsx_run_trajectories ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('member', TRAJ_MEMBERS, ids=str)
def test_scattered_trajectories_equal_the_oracle(eng, member, monkeypatch):
    set_problem(eng, *member.compiled(), monkeypatch)
    first, offsets, t_len = member.traj_list
    trajs, st = eng.trajectories(first, offsets, t_len)
    assert len(trajs) == len(offsets)
    for got, o, t in zip(trajs, offsets, t_len):
        assert np.array_equal(got, member.trajectory(first + o, t)), (o, t)
    assert st['state_steps'] == sum(t_len)


SENTINEL = 0xA5A55A5AC3C33C3C


def test_trajectories_land_where_they_are_told_and_nowhere_else(eng, monkeypatch):
    """The raw ABI with out_offsets in descending order and gaps, over a buffer filled with a sentinel (n = 130: three
    64-bit words per state, where the per-lane kernel holds four)."""
    from boolsi_amd._lib import Stats, ptr
    member = BY_NAME['var_n130']
    net, space = member.compiled()
    set_problem(eng, net, space, monkeypatch)
    W = net.n_words
    first, offsets, t_len = member.traj_list
    offsets, t_len = np.array(offsets[:64], np.uint64), np.array(t_len[:64], np.uint64)
    assert W == 3 and {0, 200} <= set(t_len.tolist())
    sizes = ((t_len + np.uint64(1)) * np.uint64(W)).astype(np.int64)
    out_off, at = np.zeros(len(sizes), np.uint64), 2
    for q in reversed(range(len(sizes))):           # the last trajectory lowest, one to three free words in front of each
        out_off[q] = at
        at += int(sizes[q]) + 1 + q % 3
    words = int(out_off[0]) + int(sizes[0])
    assert all(a > b for a, b in zip(out_off, out_off[1:])) and words % 512         # (the last word ends no page)
    out = np.full(words, SENTINEL, np.uint64)
    covered = np.zeros(words, bool)
    lib, h, st = eng._lib, eng._h, Stats()

    def call(n, offs, lens, ooff):
        return lib.bsx_run_trajectories(h, C.byref(eng.index(first)), ptr(offs) if offs is not None else None,
                                        ptr(lens) if lens is not None else None, n, ptr(out), ptr(ooff) if ooff is not None else None,
                                        C.byref(st))

    assert call(0, None, None, None) == 0 and (out == SENTINEL).all()               # n = 0: BSX_OK, nothing written
    assert call(len(sizes), offsets, t_len, None) == -1 and (out == SENTINEL).all()  # BSX_ERR_INVALID
    past = np.array([space.n_problems - first], np.uint64)
    assert call(1, past, t_len[:1].copy(), out_off[:1].copy()) == -1 and (out == SENTINEL).all()
    assert call(len(sizes), offsets, t_len, out_off) == 0
    for o, t, a, size in zip(offsets.tolist(), t_len.tolist(), out_off.tolist(), sizes.tolist()):
        assert np.array_equal(out[a:a + size].reshape(-1, W), member.trajectory(first + o, t)), (o, t)
        covered[a:a + size] = True
    assert int((~covered).sum()) >= len(sizes) and (out[~covered] == SENTINEL).all()
    assert st.as_dict()['state_steps'] == int(t_len.sum())
