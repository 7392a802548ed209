#!/usr/bin/env python3
"""Heal rate against the locate, and against the path it replaces, in one process per case: RS(10,4), 1 MiB blocks,
the dirty subset of 4096 stripes resident in HBM.

Four legs alternate within a round, all over the same selection (stripe_ids = the dirty stripes) of the big array,
each timed by HIP events after a warm-up, so box-to-box and minute-to-minute drift hits them alike:
  heal_target    ecg_heal.encode_batch with the damaged block of every stripe named;
  heal_any       ecg_heal.encode_batch, ANY mode;
  locate         ecg_locate.encode_batch -- the yardstick: the same reads and the same syndrome arithmetic;
  locate_decode  the path the heal replaces: that locate, its votes copied to the host, a verdict per stripe, and one
                 ecg.decode_batch per dirty stripe (each has its own erased block) in one batch scope.
The damage is written back outside the timed regions, before every leg that needs it (the heals and the decode path
repair it).  Cases:
  a  one 4 KiB run damaged in one data block of every dirty stripe, the block rotating over the stripes (so the
     decode path sees mixed erasure patterns);
  b  one whole data block of every dirty stripe replaced by garbage, the block rotating likewise;
  c  the same selection over all-clean stripes (the floor: the clean fast path everywhere; no decode is issued).
Each case is a fresh child process under its own time limit; the driver stops at the first one that fails.  Every
case prints ONE JSON line -- bytes read, median / min / max ms and the fraction of 8 TB/s per leg, and each heal's
time over the locate's and over the decode path's -- which the driver appends to --out.  A case asserts the reports
(every dirty stripe corrected in its block, 4096 / nearly B / no bad positions), that the stripes are the encoded
ones again after every repairing leg, and that ecg_heal.counters() moved by S_sel * B * 14 bytes per heal.  Needs
the GPU: there is no CPU path.

    python tools/heal_rate.py [--stripes 4096] [--dirty-every 8] [--block 1048576] [--rounds 20] [--warmup 3]
                              [--cases abc] [--out profiles/heal/heal_rate.jsonl] [--limit 420]
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
RUN = 4096     # case a: damaged bytes per dirty stripe
LEGS = ("heal_target", "heal_any", "locate", "locate_decode")


def run_case(args, case):
    import torch

    import ecg
    import ecg_heal
    import ecg_locate

    if not torch.cuda.is_available():
        sys.exit("heal_rate.py needs an MI355X (torch.cuda.is_available() is False)")
    torch.cuda.set_device(0)
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
    blocks = (torch.arange(D, device="cuda") % k)            # the damaged data block of dirty stripe i
    targets = blocks.to(torch.int32).contiguous()
    host_rows, host_blocks = rows.cpu().tolist(), blocks.cpu().tolist()
    lo = (B // 3) & ~15
    clean = stripes[rows, blocks].clone()                    # [D][B]: the damaged blocks as encoded
    if case == "a":
        wound = clean[:, lo:lo + RUN] ^ 0x5A
    elif case == "b":
        wound = torch.empty((D, B), dtype=torch.uint8, device="cuda")
        ecg.fill_random(wound, 0xBAD)
    report = torch.empty((D, n + 2), dtype=torch.int32, device="cuda")
    votes = torch.empty((D, n + 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def damage():
        if case == "a":
            stripes[rows, blocks, lo:lo + RUN] = wound
        elif case == "b":
            stripes[rows, blocks] = wound

    def repaired():
        return torch.equal(stripes[rows, blocks], clean)

    def heal_target():
        ecg_heal.encode_batch(k, m, M, stripes, stripe_ids=sel, targets=targets, out=report)

    def heal_any():
        ecg_heal.encode_batch(k, m, M, stripes, stripe_ids=sel, out=report)

    def locate():
        ecg_locate.encode_batch(k, m, M, stripes, stripe_ids=sel, out=votes)

    decodes = [0]

    def locate_decode():
        locate()
        v = votes.cpu().numpy()
        with ecg.batch():
            for i, s in enumerate(host_rows):
                block, _ = ecg_locate.verdict(v[i])
                if block >= 0:
                    ecg.decode_batch(k, m, M, row_k_ones, [[block]], stripes[s:s + 1])
                    decodes[0] += 1

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    def check_report(mode):
        r = report.cpu().numpy()
        if case == "c":
            assert not r.any(), f"{mode}: clean stripes reported a correction"
            return
        bad = r[:, n]
        assert (r[range(D), host_blocks] == bad).all() and not r[:, n + 1].any(), f"{mode}: a block was not corrected"
        assert r[:, :n].sum() == bad.sum()
        assert (bad == RUN).all() if case == "a" else (bad > 0.99 * B).all(), bad[:4]

    legs = {"heal_target": heal_target, "heal_any": heal_any, "locate": locate, "locate_decode": locate_decode}
    ms = {name: [] for name in LEGS}
    c0 = None
    for rnd in range(args.warmup + args.rounds):
        if rnd == args.warmup:
            torch.cuda.synchronize()
            c0, decodes[0] = ecg_heal.counters(), 0
        for name in LEGS:
            if name != "locate_decode":                      # the locate before it left the damage in place
                damage()
            torch.cuda.synchronize()
            t = timed(legs[name])
            if rnd >= args.warmup:
                ms[name].append(t)
            if rnd in (0, args.warmup + args.rounds - 1):    # outside the timed region
                if name.startswith("heal"):
                    check_report(name)
                if name != "locate":
                    assert repaired(), f"{name}: the stripes are not the encoded ones again"
    c1 = ecg_heal.counters()
    assert c1["bytes"] - c0["bytes"] == 2 * args.rounds * D * B * n, (c0, c1)
    assert c1["launches"] - c0["launches"] == 2 * args.rounds
    assert decodes[0] == (0 if case == "c" else args.rounds * D), decodes

    out = {"tool": "heal_rate", "case": case, "code": "RS(10,4)", "stripes": S, "dirty_stripes": D,
           "block_bytes": B, "rounds": args.rounds, "warmup": args.warmup, "peak_bytes_per_s": PEAK,
           "decodes_per_round": decodes[0] // args.rounds, "device": torch.cuda.get_device_name(0)}
    for name, t in ms.items():
        med = statistics.median(t)
        out[name] = {"bytes": D * B * n, "ms": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                     "frac_of_8TBps": round(D * B * n / (med * 1e-3) / PEAK, 4)}
    for h in ("heal_target", "heal_any"):
        out[h + "_time_over_locate"] = round(out[h]["ms"] / out["locate"]["ms"], 4)
        out[h + "_time_over_locate_decode"] = round(out[h]["ms"] / out["locate_decode"]["ms"], 4)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--dirty-every", type=int, default=8, help="one stripe in this many is dirty")
    ap.add_argument("--block", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heal", "heal_rate.jsonl"))
    ap.add_argument("--limit", type=int, default=420, help="seconds a case may take")
    ap.add_argument("--case", choices=["a", "b", "c"], help="run this one case in this process (the driver's child)")
    args = ap.parse_args()
    if args.case:
        return run_case(args, args.case)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for case in args.cases:
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
