#!/usr/bin/env python3
"""Restore rate against the heal's TARGET mode and against the path it replaces, in one process per case: RS(10,4),
1 MiB blocks, the dirty subset of 4096 stripes resident in HBM.

The legs alternate within a round, all over the same selection (stripe_ids = the dirty stripes) of the big array, each
timed by HIP events after a warm-up, so box-to-box and minute-to-minute drift hits them alike:
  restore        ecg_restore.encode_batch with the flagged set of every stripe (plan launch and main launch);
  heal_target    ecg_heal.encode_batch with the FIRST flagged block of every stripe named -- the yardstick: the same
                 reads and the same syndrome arithmetic.  With one flagged block it repairs what the restore repairs;
                 with more it leaves the positions alone (two damaged blocks explain no single one), and is a timing
                 yardstick only;
  heal_control   the same call again: the spread of one unchanged leg against itself;
  decode         the path the restore replaces: one ecg.decode_batch per dirty stripe with its erasures given, in one
                 batch scope (the erasure sets differ per stripe, so each is a call of its own).
The damage is written back outside the timed regions, before every leg.  Cases:
  c   clean stripes, one block flagged per stripe (the floor: the clean fast path everywhere; no decode is issued);
  a1  one 4 KiB run in the one flagged block of every dirty stripe, the block rotating over the stripes;
  a2  4 KiB runs in two flagged blocks, the set rotating;
  a4  4 KiB runs in four flagged blocks, the set rotating;
  b2  two whole flagged blocks replaced by garbage, the set rotating.
Each case is a fresh child process under its own time limit; the driver stops at the first one that fails.  Every case
prints ONE JSON line -- bytes read, median / min / max ms and the fraction of 8 TB/s per leg, the restore's time over
each yardstick's and the control's over the heal's -- which the driver appends to --out.  A case asserts the reports,
that the stripes are the encoded ones again after every repairing leg, and that ecg_restore.counters() moved by
S_sel * B * 14 bytes per call.  Needs the GPU: there is no CPU path.

    python tools/restore_rate.py [--stripes 4096] [--dirty-every 8] [--block 1048576] [--rounds 20] [--warmup 3]
                                 [--cases c,a1,a2,a4,b2] [--out profiles/restore/restore_rate.jsonl] [--limit 420]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "erasure-codes-prototype_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK = 8.0e12  # MI355X HBM3E peak, bytes per second
RUN = 4096     # damaged bytes per flagged block in the run cases
LEGS = ("restore", "heal_target", "heal_control", "decode")
CASES = {"c": (1, "clean"), "a1": (1, "run"), "a2": (2, "run"), "a4": (4, "run"), "b2": (2, "whole")}


def run_case(args, case):
    import torch

    import ecg
    import ecg_heal
    import ecg_restore

    if not torch.cuda.is_available():
        sys.exit("restore_rate.py needs an MI355X (torch.cuda.is_available() is False)")
    torch.cuda.set_device(0)
    t_flag, kind = CASES[case]
    k, m, S, B = 10, 4, args.stripes, args.block
    n = k + m
    M = ecg.reed_sol_vandermonde_coding_matrix(k, m)
    row_k_ones = int(all(v == 1 for v in M[:k]))
    stripes = torch.empty((S, n, B), dtype=torch.uint8, device="cuda")
    ecg.fill_random(stripes, 0x4EA1)
    ecg.encode_batch(k, m, M, stripes[:, :k], stripes[:, k:])
    sel = torch.arange(args.dirty_every // 2, S, args.dirty_every, dtype=torch.int32, device="cuda")
    D = int(sel.numel())
    rows = sel.long()
    # flagged block j of dirty stripe i: (i + 3 j) % n -- data and coding blocks, the set rotating over the stripes
    sets = [[(i + 3 * j) % n for j in range(t_flag)] for i in range(D)]
    named = torch.zeros((D, n), dtype=torch.uint8)
    for i, E in enumerate(sets):
        named[i, E] = 1
    named = named.cuda()
    targets = torch.tensor([E[0] for E in sets], dtype=torch.int32, device="cuda")
    host_rows = rows.cpu().tolist()
    lo = (B // 3) & ~15
    flagged = [torch.tensor([E[j] for E in sets], device="cuda") for j in range(t_flag)]
    clean = [stripes[rows, fb].clone() for fb in flagged]            # [D][B] per flagged position, as encoded
    if kind == "run":
        wound = [c[:, lo + 64 * j:lo + 64 * j + RUN] ^ (0x5A + j) for j, c in enumerate(clean)]
    elif kind == "whole":
        wound = []
        for j in range(t_flag):
            w = torch.empty((D, B), dtype=torch.uint8, device="cuda")
            ecg.fill_random(w, 0xBAD + j)
            wound.append(w)
    report = torch.empty((D, n + 3), dtype=torch.int32, device="cuda")
    hreport = torch.empty((D, n + 2), dtype=torch.int32, device="cuda")
    work = torch.empty((ecg_restore.work_bytes(D),), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def damage():
        for j, fb in enumerate(flagged):
            if kind == "run":
                stripes[rows, fb, lo + 64 * j:lo + 64 * j + RUN] = wound[j]
            elif kind == "whole":
                stripes[rows, fb] = wound[j]

    def repaired():
        return all(torch.equal(stripes[rows, fb], c) for fb, c in zip(flagged, clean))

    def restore():
        ecg_restore.encode_batch(k, m, M, stripes, named, stripe_ids=sel, work=work, out=report)

    def heal_target():
        ecg_heal.encode_batch(k, m, M, stripes, stripe_ids=sel, targets=targets, out=hreport)

    decodes = [0]

    def decode():
        if kind == "clean":
            return
        with ecg.batch():
            for i, s in enumerate(host_rows):
                ecg.decode_batch(k, m, M, row_k_ones, [sorted(sets[i])], stripes[s:s + 1])
                decodes[0] += 1

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    def check_report():
        r = report.cpu().numpy()
        assert not r[:, n + 2].any() and not r[:, n + 1].any(), "restore: a stripe was unusable or a position left"
        if kind == "clean":
            assert not r.any(), "restore: clean stripes reported a correction"
            return
        per = RUN if kind == "run" else B
        for i, E in enumerate(sets):
            got = r[i, E]
            assert (got == per).all() if kind == "run" else (got > 0.99 * B).all(), (i, E, got)
        assert r[:, :n].sum() == sum(int(r[i, E].sum()) for i, E in enumerate(sets))

    legs = {"restore": restore, "heal_target": heal_target, "heal_control": heal_target, "decode": decode}
    repairs = {"restore": True, "heal_target": t_flag == 1, "heal_control": t_flag == 1, "decode": kind != "clean"}
    ms = {name: [] for name in LEGS}
    c0 = None
    for rnd in range(args.warmup + args.rounds):
        if rnd == args.warmup:
            torch.cuda.synchronize()
            c0, decodes[0] = ecg_restore.counters(), 0
        for name in LEGS:
            damage()
            torch.cuda.synchronize()
            t = timed(legs[name])
            if rnd >= args.warmup:
                ms[name].append(t)
            if rnd in (0, args.warmup + args.rounds - 1):    # outside the timed region
                if name == "restore":
                    check_report()
                if repairs[name]:
                    assert repaired(), f"{name}: the stripes are not the encoded ones again"
    c1 = ecg_restore.counters()
    assert c1["bytes"] - c0["bytes"] == args.rounds * D * B * n, (c0, c1)
    assert c1["launches"] - c0["launches"] == args.rounds
    assert decodes[0] == (0 if kind == "clean" else args.rounds * D), decodes

    out = {"tool": "restore_rate", "case": case, "flagged_per_stripe": t_flag, "damage": kind, "code": "RS(10,4)",
           "stripes": S, "dirty_stripes": D, "block_bytes": B, "rounds": args.rounds, "warmup": args.warmup,
           "peak_bytes_per_s": PEAK, "decodes_per_round": decodes[0] // args.rounds,
           "heal_target_repairs": t_flag == 1, "device": torch.cuda.get_device_name(0)}
    for name, t in ms.items():
        med = statistics.median(t)
        nbytes = D * B * (k + t_flag if name == "decode" else n)     # a decode reads k blocks and writes t
        out[name] = {"bytes": nbytes, "ms": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                     "frac_of_8TBps": round(nbytes / (med * 1e-3) / PEAK, 4) if med > 0 else 0.0}
    out["restore_time_over_heal_target"] = round(out["restore"]["ms"] / out["heal_target"]["ms"], 4)
    out["heal_control_time_over_heal_target"] = round(out["heal_control"]["ms"] / out["heal_target"]["ms"], 4)
    if kind != "clean":
        out["restore_time_over_decode"] = round(out["restore"]["ms"] / out["decode"]["ms"], 4)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--dirty-every", type=int, default=8, help="one stripe in this many is dirty")
    ap.add_argument("--block", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="c,a1,a2,a4,b2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restore", "restore_rate.jsonl"))
    ap.add_argument("--limit", type=int, default=420, help="seconds a case may take")
    ap.add_argument("--case", choices=sorted(CASES), help="run this one case in this process (the driver's child)")
    args = ap.parse_args()
    if args.case:
        return run_case(args, args.case)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for case in args.cases.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--stripes", str(args.stripes),
               "--dirty-every", str(args.dirty_every), "--block", str(args.block), "--rounds", str(args.rounds),
               "--warmup", str(args.warmup)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"case {case} did not finish in {args.limit} s: stopping")
        if res.returncode != 0:
            sys.stderr.write(res.stdout + res.stderr)
            sys.exit(f"case {case} failed with status {res.returncode}: stopping")
        line = res.stdout.strip().splitlines()[-1]
        json.loads(line)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
