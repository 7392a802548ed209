"""Generate tests/golden/reference_ec.json from the reference's OWN EC classes.

oracle/_ref/ref_ec_cpu is the reference's unchanged project/src/ec/*.cpp compiled against include/jerasure_shim/ and
linked with oracle/ref_driver.cpp and oracle/ref_cpu_backend.c (oracle/Makefile builds it where the reference's sources
are present).  This runs it over the cases of tests/reference_ec_cases.py and records what the classes returned:
parameters, matrices, partitions and decodability flags in full; the repair plans and, of every output block, its
SHA-256 plus first 16 bytes, folded into one SHA-256 per code and group of cases (reference_ec_cases.fold), which keeps
the file in the tens of kilobytes; the SHA-256 of the five reference sources and the request's own digest.

A case at which the reference ends its own process (utils.cpp's my_assert) is recorded as "reference_exits", never
dropped; the run restarts without it.

Run:  python tests/golden/make_reference_golden.py
"""
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import reference_ec_cases as C  # noqa: E402

MAX_EXIT_SHARE = 0.02
NEEDED = ("encode", "multi_decode", "undecodable", "plan")


def answer(lines, workdir):
    """Results aligned with lines; a line the reference exits on is "reference_exits" and the run restarts without
    it."""
    out = [None] * len(lines)
    alive = list(range(len(lines)))
    while True:
        got, rc, err = C.run_driver(C.REF_CPU, [lines[i] for i in alive], workdir)
        for i, r in zip(alive, got):
            out[i] = r
        if len(got) == len(alive):
            assert rc == 0, (rc, err)
            return out
        assert rc == 1, "the driver ended with %d, not by the reference's exit: %s" % (rc, err[-2000:])
        out[alive[len(got)]] = "reference_exits"
        del alive[len(got)]


def check_conditions(codes):
    tally = C.class_tally(codes)
    cases = sum(t["cases"] for t in tally.values())
    exits = sum(t["reference_exits"] for t in tally.values())
    assert exits <= MAX_EXIT_SHARE * cases, (exits, cases)
    assert sorted(tally) == sorted(C.TYPE_NAMES.values()), sorted(tally)
    for name, t in tally.items():
        for what in NEEDED:
            assert t[what] >= 1, (name, what, t)
    return tally, cases, exits


def main():
    assert os.path.exists(C.REF_CPU), "build oracle/_ref/ref_ec_cpu first (make -C oracle, with the reference present)"
    codes = []
    with tempfile.TemporaryDirectory() as tmp:
        for inst in C.instances():
            base = C.head_lines(inst) + C.pattern_lines(inst)
            lines = C.code_lines(inst, answer(base, tmp))
            answers = answer(lines, tmp)
            assert C.code_lines(inst, answers) == lines
            codes.append((inst, lines, answers))
            print("%-40s %5d lines" % (inst["name"], len(lines)))
    tally, cases, exits = check_conditions(codes)
    rec = {"note": "written by tests/golden/make_reference_golden.py from the reference's own EC classes "
                   "(oracle/_ref/ref_ec_cpu); arithmetic underneath: oracle/jerasure_w8.c",
           "sources": {s: hashlib.sha256(open(os.path.join(C.REFERENCE, "src", "ec", s), "rb").read()).hexdigest()
                       for s in C.REF_SOURCES},
           "cases": cases, "reference_exits": exits, "tally": tally,
           "codes": [dict(inst, **C.fold(lines, answers)) for inst, lines, answers in codes]}
    rec["request_sha256"] = hashlib.sha256("".join(c["request_sha256"] for c in rec["codes"]).encode()).hexdigest()
    with open(C.RECORD, "w") as f:
        f.write("{\n")
        for key in [k for k in rec if k != "codes"]:
            f.write(" %s: %s,\n" % (json.dumps(key), json.dumps(rec[key])))
        f.write(' "codes": [\n  %s\n ]\n}\n' % ",\n  ".join(C.canonical(c) for c in rec["codes"]))
    json.load(open(C.RECORD))
    print("wrote %s: %d bytes, %d cases, %d reference_exits" % (C.RECORD, os.path.getsize(C.RECORD), cases, exits))
    for name, t in tally.items():
        print("  %-20s %s" % (name, t))


if __name__ == "__main__":
    main()
