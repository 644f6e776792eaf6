"""Host layers of the wide-state family (no GPU): compile of a 1024-node network, the ATTR_REC2W record layout
against include/bsx.h, and merging of wide records by their integer key."""
import os
import re

import numpy as np
import pytest

from boolsi_amd import _lib, synth
from boolsi_amd.attract import merge_tables, table_from_merged
from boolsi_amd.compile import MAX_NODES, compile_problem
from boolsi_amd.constants import Mode
from boolsi_amd.input import parse_input_text

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'bsx.h')


def _define(name):
    with open(HEADER) as f:
        return int(re.search(r'#define\s+{}\s+(\d+)'.format(name), f.read()).group(1))


def test_constants_match_the_header():
    assert _lib.MAX_NODES_WIDE == _define('BSX_MAX_NODES_WIDE') == MAX_NODES == 1024
    assert _lib.MAX_STATE_WORDS == _define('BSX_MAX_STATE_WORDS') == 16
    assert _lib.LUT_WIDE == _define('BSX_LUT_WIDE')
    assert _lib.MAX_NODES == _define('BSX_MAX_NODES') == 256
    assert 'bsx_run_attract_wide' in _lib.EXPORTS


def test_attr_rec2w_layout():
    # key[16], length, bsx_u128 count, sum_l[3], sum_l2[4]: 8-byte fields, no padding
    assert _lib.ATTR_REC2W.itemsize == 8 * (16 + 1 + 2 + 3 + 4)
    assert [_lib.ATTR_REC2W.fields[n][1] for n in ('key', 'length', 'count', 'sum_l', 'sum_l2')] == [0, 128, 136, 152, 176]
    assert _lib.ATTR_REC2W.fields['count'][0] == _lib.ATTR_REC2.fields['count'][0]


def test_compile_1024_node_network():
    n = 1024
    cfg = parse_input_text(synth.network_yaml(n, 3, 9, initial={i: '0' for i in range(8, n)}), 100, Mode.ATTRACT)
    net, space = compile_problem(cfg)
    assert net.n_nodes == n and net.n_words == 16
    assert len(space.any_nodes) == 8
    with pytest.raises(ValueError, match='more than 1024 nodes'):
        text = synth.network_yaml(n + 1, 2, 9, initial={i: '0' for i in range(n + 1)})
        compile_problem(parse_input_text(text, 100, Mode.ATTRACT))


def test_wide_records_merge_by_integer_key():
    big = (1 << 1000) | 12345
    t = np.zeros(3, _lib.ATTR_REC2W)
    for i, (key, cnt, sl, sl2) in enumerate([(big, 2, 10, 50), (7, 1, 3, 9), (big, 3, 1, 1)]):
        for w in range(16):
            t[i]['key'][w] = (key >> (64 * w)) & (2 ** 64 - 1)
        t[i]['length'] = 4
        t[i]['count'][0], t[i]['sum_l'][0], t[i]['sum_l2'][0] = cnt, sl, sl2
    merged = merge_tables([t[:2], t[2:]])
    assert merged == {big: [4, 5, 11, 51], 7: [4, 1, 3, 9]}
    back = table_from_merged(merged, _lib.ATTR_REC2W)
    assert merge_tables([back]) == merged
    with pytest.raises(OverflowError):
        table_from_merged(merged, _lib.ATTR_REC2)
