"""Kernel resources of libecg_vread.so, read from its gfx950 code-object metadata as tests/test_kernel_resources.py reads
libecg.so's (CPU only): the family of kernels, no private segment, no VGPR spills, LDS for the CRC tables only.
"""
import os
import re

import pytest

import test_kernel_resources as KR

LIB = os.path.join(os.path.dirname(KR.LIB), "libecg_vread.so")
TABLE_BYTES = 4 * 256 * 4                                  # psum_kernels.hpp kPsumTableWords words


@pytest.fixture(scope="module")
def meta():
    assert os.path.exists(LIB), "libecg_vread.so not built"
    saved = KR.LIB
    KR.LIB = LIB
    try:
        return KR._metadata()
    finally:
        KR.LIB = saved


def _short(meta):
    return {re.search(r"gf_vread_\w*?kernel", s).group(0): f for s, f in meta.items()}


def test_code_object_is_the_vread_family(meta):
    assert sorted(_short(meta)) == ["gf_vread_byte_kernel", "gf_vread_plan_kernel", "gf_vread_rows_kernel",
                                    "gf_vread_small_kernel", "gf_vread_verdict_kernel"], list(meta)


def test_no_private_segment_and_no_vgpr_spills(meta):
    bad = {n: f for n, f in meta.items() if f.get("private_segment_fixed_size", 0) or f.get("vgpr_spill_count", 0)}
    assert not bad, bad
    assert all(f["kernarg_segment_size"] <= 4096 for f in meta.values())
    assert max(f["vgpr_count"] for f in meta.values()) <= 256


def test_lds_holds_the_crc_tables_only(meta):
    lds = {n: f.get("group_segment_fixed_size", 0) for n, f in _short(meta).items()}
    assert lds == {"gf_vread_plan_kernel": 0, "gf_vread_byte_kernel": 0, "gf_vread_verdict_kernel": 0,
                   "gf_vread_small_kernel": 7 * TABLE_BYTES, "gf_vread_rows_kernel": 9 * TABLE_BYTES}, lds
