"""The oracle's restatement and the product's host-side facade against the reference's OWN EC classes (CPU).

tests/golden/reference_ec.json records what the reference's unchanged erasure_code.cpp / rs.cpp / lrc.cpp / pc.cpp
returned for the cases of tests/reference_ec_cases.py (tests/golden/make_reference_golden.py wrote it from
oracle/_ref/ref_ec_cpu): parameters, matrices, FLAT and OPTIMAL partitions and decodability flags in full, repair plans
(field for field, in order) and every output block's digest as one SHA-256 per code and group of cases.  Everything here
is exact.  oracle/ec_ref.py and oracle/plan_ref.py are what every GPU byte is compared with, so this is the test that
pins them; the facade's host-side answers (no GPU needed) are held to the same record.
"""
import json
import os

import pytest

import reference_ec_cases as C
import reference_ec_replay as R

RECORD = json.load(open(C.RECORD))
CODES = RECORD["codes"]
IDS = [c["name"] for c in CODES]
INPUT = C.input_bytes()


@pytest.mark.parametrize("code", CODES, ids=IDS)
def test_oracle_matches_reference(oracle, code):
    """ec_ref.py / plan_ref.py recompute every recorded case: k, m, matrix, partitions, flags, then plans and every
    output block's digest through the groups' digests."""
    o, stripes = R.OracleSubject(code), {}
    lines, answers = R.request_of(code, o, INPUT, stripes)
    got = R.folded(code, lines, answers + R.replay(o, lines[len(answers):], INPUT, stripes=stripes))
    for key in ("k", "m", "matrix", "partition", "flags", "request_sha256", "sha256"):
        assert got[key] == code[key], key


@pytest.mark.parametrize("code", CODES, ids=IDS)
def test_facade_host_side_matches_reference(ecg, oracle, code):
    """The facade's ecg_ec_k / ecg_ec_m / ecg_ec_get_coding_parameters, ecg_ec_make_encoding_matrix, ecg_ec_get_partition
    after generate_partition and ecg_ec_check_if_decodable equal the record; ecg_ec_generate_repair_plan equals, plan for
    plan, the oracle's answers that test_oracle_matches_reference holds to the record's digests; and the coefficients
    of ecg_ec_partial_decoding_matrix / ecg_ec_partial_encoding_matrix turn the recorded calls' input blocks into the
    same output blocks."""
    facade = R.FacadeSubject(code)
    cp = facade.ec.get_coding_parameters()
    for field, ref_value in zip(C.CP_FIELDS + ("local_or_column",), code["cp"]):
        if ref_value != -1:  # a field the reference's class owns
            assert int(getattr(cp, field)) == ref_value, (field, ref_value)
    base = C.head_lines(code) + C.pattern_lines(code)
    answers = R.replay(facade, base, INPUT, with_bytes=False)
    got = R.folded(code, base, answers)
    for key in ("k", "m", "matrix", "partition", "flags"):
        assert got[key] == code[key], key
    o, stripes = R.OracleSubject(code), {}
    lines, ref = R.request_of(code, o, INPUT, stripes)
    assert C.fold(lines, ref)["request_sha256"] == code["request_sha256"]
    for line, g, r in zip(base, answers, ref):
        if line.startswith("pat"):
            assert (g["ret"], g["plans"]) == (r["ret"], r["plans"]), line
    partial = lines[len(base):]
    for line, r in zip(partial, R.replay(o, partial, INPUT, stripes=stripes)):
        assert R.partial_matrix_outputs(facade, oracle, line, stripes) == r, line


def test_record_conditions():
    """The record's own conditions: its codes are the ones the helper names now, at most 2 % of its cases are ones the
    reference exits on, and each of the ten classes keeps an encode, a decodable multi-block decode, an undecodable flag
    and a repair plan."""
    assert [(c["name"], c["type"], c["params"], c["isvertical"]) for c in CODES] == \
           [(i["name"], i["type"], i["params"], i["isvertical"]) for i in C.instances()]
    tally = RECORD["tally"]
    cases = sum(t["cases"] for t in tally.values())
    exits = sum(t["reference_exits"] for t in tally.values())
    assert cases == RECORD["cases"] and exits == RECORD["reference_exits"] == sum(len(c["exits"]) for c in CODES)
    assert exits <= 0.02 * cases, (exits, cases)
    assert sorted(tally) == sorted(C.TYPE_NAMES.values())
    for name, t in tally.items():
        for what in ("encode", "multi_decode", "undecodable", "plan"):
            assert t[what] >= 1, (name, what)
        mine = [c for c in CODES if C.TYPE_NAMES[c["type"]] == name]
        assert t["undecodable"] == sum(c["flags"].count("0") for c in mine), name
        assert all(len(c["flags"]) == len(C.pattern_lines(c)) for c in mine), name
    assert os.path.getsize(C.RECORD) < 128 << 10


HAVE_REFERENCE = os.path.isdir(os.path.join(C.REFERENCE, "src", "ec")) and os.path.exists(C.REF_CPU)
needs_reference = pytest.mark.skipif(not HAVE_REFERENCE, reason="needs the reference's sources and the built "
                                     "oracle/_ref/ref_ec_cpu (build container only)")


@needs_reference
def test_record_names_these_reference_sources():
    import hashlib
    for src, sha in RECORD["sources"].items():
        with open(os.path.join(C.REFERENCE, "src", "ec", src), "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == sha, src
    assert sorted(RECORD["sources"]) == sorted(C.REF_SOURCES)


def _run_all(binary, per_code_lines, workdir, timeout):
    """One process over every code's lines; the answers per code."""
    lines = [l for ls in per_code_lines for l in ls]
    got, rc, err = C.run_driver(binary, lines, workdir, timeout=timeout)
    assert rc == 0 and len(got) == len(lines), (rc, len(got), len(lines), err[-2000:])
    it = iter(got)
    return [[next(it) for _ in ls] for ls in per_code_lines]


@needs_reference
def test_rerun_reproduces_record(tmp_path):
    """One process of the reference binary over the whole request (less the cases it exits on) answers what the record
    holds, and its tally is the recorded one."""
    base = _run_all(C.REF_CPU, [C.head_lines(c) + C.pattern_lines(c) for c in CODES], str(tmp_path), 120)
    lines = [C.code_lines(c, a) for c, a in zip(CODES, base)]
    kept = [C.kept_lines(ls, c) for ls, c in zip(lines, CODES)]
    answers = [C.with_exits(ls, c, a) for ls, c, a in zip(lines, CODES, _run_all(C.REF_CPU, kept, str(tmp_path), 120))]
    for c, ls, a in zip(CODES, lines, answers):
        assert dict(c, **C.fold(ls, a)) == c, c["name"]
    assert C.class_tally(zip(CODES, lines, answers)) == RECORD["tally"]
