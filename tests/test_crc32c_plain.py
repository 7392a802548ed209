"""tests/crc32c_plain.py against the known answers of include/ecg_sum.h, and its numpy form against its bitwise one."""
import os
import re

import numpy as np

import crc32c_plain as CP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_known_answers():
    for data, want in CP.KNOWN:
        assert CP.bitwise(data) == want, (data, hex(CP.bitwise(data)))
        assert int(CP.many(np.frombuffer(data, dtype=np.uint8))) == want


def test_the_header_states_the_same_answers():
    hdr = open(os.path.join(ROOT, "include", "ecg_sum.h")).read()
    stated = {int(v, 16) for v in re.findall(r"0x[0-9A-F]{8}\b", hdr)}
    assert {want for _, want in CP.KNOWN if want} <= stated
    assert {0x1EDC6F41, 0x82F63B78, 0xFFFFFFFF} <= stated


def test_numpy_form_equals_the_bitwise_form():
    rng = np.random.default_rng(32)
    for B in list(range(0, 20)) + [int(v) for v in rng.integers(20, 71, 12)]:
        blocks = rng.integers(0, 256, (3, 2, B), dtype=np.uint8)
        got = CP.many(blocks)
        assert got.shape == (3, 2) and got.dtype == np.uint32
        for i in range(3):
            for j in range(2):
                assert int(got[i, j]) == CP.bitwise(blocks[i, j].tobytes()), (B, i, j)


def test_numpy_form_with_a_length_per_row():
    rng = np.random.default_rng(33)
    blocks = rng.integers(0, 256, (40, 70), dtype=np.uint8)
    lengths = rng.integers(0, 71, 40)
    lengths[:3] = (0, 70, 1)
    got = CP.many(blocks, lengths)
    for r in range(40):
        assert int(got[r]) == CP.bitwise(blocks[r, :lengths[r]].tobytes()), (r, lengths[r])


def test_table_is_the_one_byte_remainder():
    assert int(CP.TABLE[0]) == 0 and int(CP.TABLE[128]) == CP.POLY
    assert len(set(int(v) for v in CP.TABLE)) == 256
