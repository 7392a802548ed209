"""The cases of the reference-EC record (tests/golden/reference_ec.json), shared by its maker
(tests/golden/make_reference_golden.py), tests/test_reference_ec.py and tests/test_gpu_reference_ec.py.

Imports nothing of the project.  It names the codes, the erasure patterns and the partial-coding arguments, writes
them as the request oracle/ref_driver.cpp reads, runs that driver and folds its answers into the record's form.
"""
import hashlib
import itertools
import json
import os
import random
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RECORD = os.path.join(HERE, "golden", "reference_ec.json")
REF_CPU = os.path.join(ROOT, "oracle", "_ref", "ref_ec_cpu")
REF_GPU = os.path.join(ROOT, "oracle", "_ref", "ref_ec_gpu")
REFERENCE = "/root/reference/project"
REF_SOURCES = ["erasure_code.cpp", "rs.cpp", "lrc.cpp", "pc.cpp", "utils.cpp"]

SIZES = (80, 1029)      # whole 16-byte columns only; vector part plus a 5-byte tail
SLOT = 1029             # data block i of size B is INPUT[i * SLOT : i * SLOT + B]
ERASED = 0xE7           # what an erased block holds before a decode
MULTI_SAMPLE = 40       # seeded multi-block patterns per code
CP_FIELDS = ("k", "m", "l", "g", "k1", "m1", "k2", "m2", "x", "seri_num")
TYPE_NAMES = {0: "RS", 1: "ERS", 2: "AZURE_LRC", 3: "AZURE_LRC_1", 4: "OPTIMAL_LRC", 5: "OPTIMAL_CAUCHY_LRC",
              6: "UNIFORM_CAUCHY_LRC", 7: "PC", 8: "Hierachical_PC", 9: "HV_PC"}


def _random_configs(n, seed):
    """Random valid parameters for every ECTYPE (divisibility kept so groups are whole; Cauchy LRCs with
    g >= 2 since g = 1 needs the unpinned cbest_8 table)."""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        t = rng.randrange(10)
        if t == 0:
            p = dict(k=rng.randint(1, 40), m=rng.randint(1, 8))
        elif t == 1:
            x = rng.randint(2, 4)
            p = dict(k=rng.randint(2, 12), m=rng.randint(1, 4), x=x, seri_num=rng.randrange(x))
        elif t in (2, 5):  # Azure, Optimal-Cauchy: l | k
            l = rng.randint(1, 4)
            p = dict(k=l * rng.randint(2, 6), l=l, g=rng.randint(2 if t == 5 else 1, 4))
        elif t == 3:       # Azure+1: (l - 1) | k
            l = rng.randint(2, 4)
            p = dict(k=(l - 1) * rng.randint(2, 6), l=l, g=rng.randint(1, 3))
        elif t in (4, 6):  # Optimal, Uniform-Cauchy: l | (k + g)
            l = rng.randint(1, 4)
            g = rng.randint(2 if t == 6 else 1, 4)
            kg = l * rng.randint(max(2, (g + 2 + l - 1) // l), 6)
            p = dict(k=kg - g, l=l, g=g)
        else:              # PC, HPC, HVPC
            p = dict(k1=rng.randint(2, 5), m1=rng.randint(1, 2), k2=rng.randint(2, 4), m2=rng.randint(1, 2))
            if t == 8:
                p.update(x=rng.randint(2, 3), seri_num=0)
                p["seri_num"] = rng.randrange(p["x"])
        out.append((f"rand{len(out)}-{t}-{p}", t, p))
    return out


def input_bytes():
    """64 KiB of SHA-256 counter-mode bytes: the one binary input every data block is cut from."""
    return b"".join(hashlib.sha256(b"reference-ec-input-%d" % i).digest() for i in range(2048))


def data_block(inp, i, B):
    return inp[i * SLOT:i * SLOT + B]


def full_params(t, p):
    """All ten CodingParameters fields, k and m as the class computes them where it owns them."""
    q = {f: 0 for f in CP_FIELDS}
    q.update(p)
    if 2 <= t <= 6:
        q["m"] = q["l"] + q["g"]
    if t >= 7:
        q["k"] = q["k1"] * q["k2"]
        q["m"] = (q["k1"] + q["m1"]) * (q["k2"] + q["m2"]) - q["k"]
    return q


def block_count(t, q):
    if t == 9:
        return q["k"] + q["k1"] * q["m2"] + q["k2"] * q["m1"]
    return q["k"] + q["m"]


def fault_tolerance(t, q):
    """Failures every pattern of which the code survives: m for RS, g + 1 for the LRCs (distance g + 2), the grid's
    (m1 + 1)(m2 + 1) - 1 for PC and m1 + m2 without the global parities."""
    if t <= 1:
        return q["m"]
    if t <= 6:
        return q["g"] + 1
    if t == 9:
        return q["m1"] + q["m2"]
    return (q["m1"] + 1) * (q["m2"] + 1) - 1


def instances():
    """Every code instance of the record: the 17 of golden.json, the first 30 random configurations and PC, HPC,
    HVPC at (4,1,4,1) and (3,2,3,2); ERS and HPC at every seri_num, HPC with isvertical both ways."""
    golden = json.load(open(os.path.join(HERE, "golden", "golden.json")))["codes"]
    base = [(c["name"], c["type"], c["params"]) for c in golden]
    base += _random_configs(60, 0xC0DE5)[:30]
    for dims in ((4, 1, 4, 1), (3, 2, 3, 2)):
        p = dict(zip(("k1", "m1", "k2", "m2"), dims))
        base += [("PC%s" % (dims,), 7, p), ("HPC%s" % (dims,), 8, dict(p, x=2, seri_num=0)), ("HVPC%s" % (dims,), 9, p)]
    out, seen = [], set()
    for name, t, p in base:
        if t in (5, 6) and p["g"] + 1 == 2:  # cauchy_good_general_coding_matrix(k, 2): refused as ECG_EUNPINNED
            continue
        for seri in (range(p["x"]) if t in (1, 8) else [None]):
            for isv in ((1, 0) if t == 8 else (1,)):
                q = full_params(t, p if seri is None else dict(p, seri_num=seri))
                key = (t, tuple(q[f] for f in CP_FIELDS), isv)
                if key in seen:
                    continue
                seen.add(key)
                label = name if seri is None or seri == p["seri_num"] else f"{name}@seri{seri}"
                out.append({"name": label + ("" if isv else "@horizontal"), "type": t, "params": q, "isvertical": isv,
                            "exhaustive": t >= 7 and (q["k1"], q["m1"], q["k2"], q["m2"]) == (4, 1, 4, 1)})
    return out


def patterns(inst):
    """(singles, multis): every single block; a seeded sample of MULTI_SAMPLE patterns of 2 up to (fault tolerance
    + 1) blocks, every other one of the largest size (where undecodable ones are); for the (4,1,4,1) product codes,
    every pattern of 2 and 3 in place of the sampled ones of those sizes."""
    t, q = inst["type"], inst["params"]
    n = block_count(t, q)
    singles = [[i] for i in range(n)]
    top = min(fault_tolerance(t, q) + 1, n)
    rng = random.Random("patterns:" + inst["name"])
    multis, seen = [], set()
    want = [top if i % 2 == 0 else rng.randint(2, top) for i in range(MULTI_SAMPLE)] if top >= 2 else []
    for size in want:
        for _ in range(20):
            pat = tuple(sorted(rng.sample(range(n), min(size, n))))
            if pat not in seen:
                seen.add(pat)
                multis.append(list(pat))
                break
    if t >= 7:  # random patterns almost never block a grid: put the smallest pattern that does in front
        multis = [stuck_pattern(t, q)] + [p for p in multis if p != stuck_pattern(t, q)]
    if inst["exhaustive"]:
        multis = [list(c) for size in (2, 3) for c in itertools.combinations(range(n), size)] + \
                 [p for p in multis if len(p) > 3]
    return singles, multis


def bid2rowcol(q, bid):
    """The product codes' block numbering: data, row parities, column parities, global parities."""
    k1, m1, k2, m2 = q["k1"], q["m1"], q["k2"], q["m2"]
    if bid < k1 * k2:
        return bid // k1, bid % k1
    if bid < (k1 + m1) * k2:
        return (bid - k1 * k2) // m1, (bid - k1 * k2) % m1 + k1
    if bid < (k1 + m1) * k2 + k1 * m2:
        return (bid - (k1 + m1) * k2) // k1 + k2, (bid - (k1 + m1) * k2) % k1
    rest = bid - (k1 + m1) * k2 - k1 * m2
    return rest // m1 + k2, rest % m1 + k1


def rowcol2bid(q, row, col):
    k1, m1, k2, m2 = q["k1"], q["m1"], q["k2"], q["m2"]
    if row < k2:
        return row * k1 + col if col < k1 else k1 * k2 + row * m1 + col - k1
    if col < k1:
        return (k1 + m1) * k2 + (row - k2) * k1 + col
    return (k1 + m1) * k2 + k1 * m2 + (row - k2) * m1 + col - k1


def stuck_pattern(t, q):
    """The smallest undecodable pattern of a product code, (fault tolerance + 1) blocks: with global parities an
    (m2 + 1) x (m1 + 1) corner of the grid, where every row and column it touches has lost one block too many; without
    them block 0, its row's parities and its column's parities, which no other row or column covers."""
    if t == 9:
        return sorted([0] + [rowcol2bid(q, 0, q["k1"] + j) for j in range(q["m1"])] +
                      [rowcol2bid(q, q["k2"] + j, 0) for j in range(q["m2"])])
    return sorted(rowcol2bid(q, r, c) for r in range(q["m2"] + 1) for c in range(q["m1"] + 1))


def partial_args(inst, plan):
    """The partial-decoding and partial-encoding arguments one recorded repair plan gives: the first help group is the
    local survivors, the union is the survivors.  Partial decoding inverts a square matrix of the survivors' rows, so it
    is asked for only where the plan names exactly as many survivors as that matrix has rows (an LRC's local repair
    sizes the matrix by its survivors).  Partial encoding reads the first group's data blocks into the parities among
    the plan's blocks.  Returns (pdec or None, penc or None) as lists of index lists."""
    t, q = inst["type"], inst["params"]
    loc, fails, helps = plan
    if not helps or not helps[0]:
        return None, None
    first = list(helps[0])
    surv = [b for h in helps for b in h]
    members = surv + list(fails)
    if t >= 7:
        axis = 0 if loc else 1  # a column repair codes along the rows' index, a row repair along the columns'
        need = q["k2"] if loc else q["k1"]
        is_data = lambda b: bid2rowcol(q, b)[axis] < need  # noqa: E731
    elif t >= 2 and loc:
        need = len(surv)
        is_data = lambda b: b < q["k"] + q["g"]  # noqa: E731
    else:
        need = q["k"]
        is_data = lambda b: b < q["k"]  # noqa: E731
    pdec = [first, surv, list(fails)] if len(surv) == need else None
    data = [b for b in first if is_data(b)]
    par = sorted(b for b in members if not is_data(b))
    penc = [data, par] if data and par else None
    return pdec, penc


def _ints(v):
    return "%d %s" % (len(v), " ".join(map(str, v))) if v else "0"


def head_lines(inst):
    q = inst["params"]
    n = block_count(inst["type"], q)
    add = (4, 2) if n >= 4 else (2, 1)
    lines = ["code %d %s %d" % (inst["type"], " ".join(str(q[f]) for f in CP_FIELDS), inst["isvertical"]),
             "mat", "part F", "part O"]
    for B in SIZES:
        lines += ["enc %d" % B, "add %d %d %d" % (B, add[0], add[1])]
    return lines


def pattern_lines(inst):
    """Every single block under OPTIMAL and under FLAT placement (decoded once), then the multi-block patterns under
    OPTIMAL; decodes at both sizes."""
    singles, multis = patterns(inst)
    return (["pat O 3 %s" % _ints(p) for p in singles] + ["pat F 0 %s" % _ints(p) for p in singles] +
            ["pat O 3 %s" % _ints(p) for p in multis])


def partial_lines(inst, pat_lines, pat_results):
    """pdec / penc lines from the plans returned for the OPTIMAL pattern lines, plan by plan, the block size
    alternating so that both sizes carry both operations.  The exhaustive sets give partial lines for their
    single-block plans only."""
    out, turn = [], 0
    for line, res in zip(pat_lines, pat_results):
        if not line.startswith("pat O") or not isinstance(res, dict):
            continue
        if inst["exhaustive"] and int(line.split()[3]) > 1:
            continue
        for plan in res["plans"]:
            pdec, penc = partial_args(inst, plan)
            B = SIZES[turn % 2]
            turn += 1
            if pdec:
                out.append("pdec %d %d %s %s %s" % (B, plan[0], _ints(pdec[0]), _ints(pdec[1]), _ints(pdec[2])))
            if penc:
                out.append("penc %d %d %s %s" % (B, plan[0], _ints(penc[0]), _ints(penc[1])))
    return out


def code_lines(inst, results):
    """One code's request: the head, the patterns, then the partial lines that the plans in results (answers to the
    head and pattern lines, from the reference or from a subject that must agree with it) give."""
    base = head_lines(inst) + pattern_lines(inst)
    return base + partial_lines(inst, base, results[:len(base)])


def run_driver(binary, lines, workdir, timeout=600):
    """Runs the driver over the lines; returns (parsed results, as many as it answered; return code; stderr)."""
    req, inp, res = (os.path.join(workdir, f) for f in ("request.txt", "input.bin", "result.jsonl"))
    with open(req, "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(inp, "wb") as f:
        f.write(input_bytes())
    if os.path.exists(res):
        os.remove(res)
    p = subprocess.run([binary, req, inp, res], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True,
                       timeout=timeout)
    got = []
    if os.path.exists(res):
        with open(res) as f:
            got = [json.loads(x) for x in f.read().splitlines() if x.endswith("}")]
    return got, p.returncode, p.stderr


def canonical(obj):
    return json.dumps(obj, separators=(",", ":"))


def _sha(texts):
    return hashlib.sha256("\n".join(texts).encode()).hexdigest()


GROUPS = {"enc": "encode", "add": "encode", "pdec": "partials", "penc": "partials"}


def fold(lines, answers):
    """One code's answers in the record's form.  In full: k, m, the coding parameters, the matrix (None where the class
    writes none, pc.h:35), the FLAT and OPTIMAL partitions and every pattern's decodability flag.  Everything else --
    each repair plan field by field, and of every output block its SHA-256 and first 16 bytes -- as one SHA-256 per
    group of lines over the answers' canonical JSON, which a subject reproduces only by giving every one of those
    answers exactly.  An answer is "reference_exits" where the reference ended its process on the line; a subject with
    no coding parameters to show leaves cp out."""
    e = {"request_sha256": _sha(lines), "exits": [i for i, a in enumerate(answers) if a == "reference_exits"],
         "flags": "", "partition": {}}
    groups = {}
    for line, a in zip(lines, answers):
        w = line.split()
        if a == "reference_exits":
            e["flags"] += "x" if w[0] == "pat" else ""
        elif w[0] == "code":
            e.update({k: a[k] for k in ("k", "m", "cp") if k in a})
        elif w[0] == "mat":
            e["matrix"] = None if a["matrix"] is None or set(a["matrix"]) == {-1} else a["matrix"]
        elif w[0] == "part":
            e["partition"][w[1]] = a["partition"]
        elif w[0] == "pat":
            e["flags"] += str(a["dec"])
            groups.setdefault("singles" if w[3] == "1" else "multis", []).append(canonical(a))
        elif w[0] in GROUPS:
            groups.setdefault(GROUPS[w[0]], []).append(canonical(a))
    e["sha256"] = {g: _sha(v) for g, v in sorted(groups.items())}
    return e


def kept_lines(lines, entry):
    """The request without the lines at which the reference ended its process."""
    return [l for i, l in enumerate(lines) if i not in entry["exits"]]


def with_exits(lines, entry, answers):
    """Answers to kept_lines, spread back over all the lines."""
    it = iter(answers)
    return ["reference_exits" if i in entry["exits"] else next(it) for i in range(len(lines))]


def class_tally(codes):
    """Per ECTYPE name: how many encodes, decodable multi-block decodes, undecodable flags and repair plans the answers
    hold, and how many cases the reference exited on.  codes: (instance, lines, answers)."""
    tally = {}
    for inst, lines, answers in codes:
        t = tally.setdefault(TYPE_NAMES[inst["type"]], {"cases": 0, "encode": 0, "multi_decode": 0, "undecodable": 0,
                                                        "plan": 0, "reference_exits": 0})
        t["cases"] += len(lines)
        for line, r in zip(lines, answers):
            if r == "reference_exits":
                t["reference_exits"] += 1
            elif line.startswith("enc"):
                t["encode"] += 1
            elif line.startswith("pat"):
                t["multi_decode"] += 1 if int(line.split()[3]) > 1 and r["dec"] and r["d"] else 0
                t["undecodable"] += 0 if r["dec"] else 1
                t["plan"] += 1 if r["plans"] else 0
    return tally
