"""The kernel instantiations of libecg.so's gfx950 code object against the enumeration derived from the
dispatcher's constants (tests/gf_kernel_cases.py), and the sweep's declared coverage of it (CPU only).

A new instantiation fails here until tests/gf_kernel_cases.py enumerates it and a case of the GPU sweep
(tests/test_gpu_kernel_matrix.py) declares a call that launches it.
"""
import os
import re

import pytest

import gf_kernel_cases as C
from test_kernel_resources import LIB, _metadata


@pytest.fixture(scope="module")
def symbols():
    if not os.path.exists(LIB):
        pytest.skip("libecg.so not built")
    return sorted(_metadata())


def _keys_of(symbols):
    """(keys, leftover symbols) from the mangled template arguments."""
    keys, rest = [], []
    for s in symbols:
        v = re.search(r"gf_vec_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])EE", s)
        b = re.search(r"gf_byte_kernelILi(\d+)ELi(\d+)ELb([01])EE", s)
        l = re.search(r"gf_lat_dword_kernelILi(\d+)ELb([01])ELi(\d+)ELb([01])EE", s)
        if v:  # <MT, MODE, NT, BIN>
            mt, mode, nt, bn = map(int, v.groups())
            keys.append(("vec", mode, bn, nt, mt))
        elif b:  # <MT, MODE, BIN>
            mt, mode, bn = map(int, b.groups())
            keys.append(("byte", mode, bn, mt))
        elif l:  # <MT, BIN, KB, EAGER>
            mt, bn, kb, eager = map(int, l.groups())
            keys.append(("lat", bn, mt, kb, eager))
        else:
            rest.append(s)
    return keys, rest


def test_enumeration_matches_code_object(symbols):
    keys, rest = _keys_of(symbols)
    assert len(keys) == len(set(keys))
    want = C.enumeration()
    assert set(keys) - want == set(), sorted(set(keys) - want)[:8]   # built, not enumerated
    assert want - set(keys) == set(), sorted(want - set(keys))[:8]   # enumerated, not built
    count = {f: sum(k[0] == f for k in keys) for f in ("vec", "byte", "lat")}
    assert count == {"vec": 288, "byte": 72, "lat": 192}, count
    # nothing else in the code object but the resident call worker and the synthetic-data fill
    assert len(rest) == len(C.OTHER_KERNELS), rest
    for name in C.OTHER_KERNELS:
        assert sum(name in s for s in rest) == 1, (name, rest)


def test_histogram_slots_are_the_enumeration(ecg):
    """Every enumerated key has exactly one histogram slot (include/ecg.h ECG_HIST_*); the other slots are the
    combinations the header says are not built."""
    slot_of = {}
    for i in range(ecg.ECG_HIST_SLOTS):
        slot_of.setdefault(ecg.hist_key(i), []).append(i)
    assert all(len(v) == 1 for v in slot_of.values())
    assert C.enumeration() <= set(slot_of)
    spare = set(slot_of) - C.enumeration()
    for key in spare:
        if key[0] == "vec":
            _, mode, binary, nt, mt = key
            assert mt > C.K_MAX_MT and (not binary or nt != C.WIDE_BIN_NT), key
        else:
            assert key[0] == "byte" and key[3] > C.K_MAX_MT and not key[2], key
    assert tuple(ecg.LAT_BUCKETS) == C.LAT_BUCKETS
    assert ecg.lib().ecg_launch_histogram(None, 0) == ecg.ECG_HIST_SLOTS  # no GPU needed to read it
    assert ecg.lib().ecg_launch_histogram(None, 4) == ecg.ECG_EINVAL
    assert isinstance(ecg.launch_histogram(), dict)


def test_sweep_declares_every_instantiation():
    """The union of the keys the sweep's cases declare covers the enumeration; what no public call can reach
    is listed in UNREACHABLE with the routing line that makes it so, and only that."""
    declared = C.declared_keys()
    want = C.enumeration()
    assert not set(C.UNREACHABLE) - want
    assert not set(C.UNREACHABLE) & declared
    missing = want - declared - set(C.UNREACHABLE)
    assert not missing, sorted(missing)[:16]
    assert declared <= want, sorted(declared - want)[:8]
