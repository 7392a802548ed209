#!/usr/bin/env python3
"""Two-block correction against the heal, in one process per case: RS(10,4), 1 MiB blocks, the dirty subset of 4096
stripes resident in HBM (tools/heal_rate.py is the model).

The legs of a case alternate within a round, all over the same selection (stripe_ids = the dirty stripes) of the big
array, each timed by HIP events after a warm-up, so box-to-box and minute-to-minute drift hits them alike (--rotate N starts
every round with the case's N-th leg instead: a leg's place in the round is part of what it measures).  The damage
is written back outside the timed regions, before every leg.  Cases and legs:
  a  one 4 KiB run in one data block of every dirty stripe, the block rotating over the stripes:
       heal_any, heal2_any, and heal_any_c1, heal_any_c2 -- the control: the yardstick against itself.  heal2 reads
       the same bytes and must not enter its pair phase, so it should cost what heal_any costs; the margin is the
       spread the control shows in this very process (profiles/check_shared/README.md on why no fixed percentage);
  c  the same selection over all-clean stripes, the same four legs;
  d  4 KiB runs in TWO blocks of every dirty stripe at the same offsets:
       heal2_any, and locate_decode2 -- the same run's ecg_locate.encode_batch plus one two-erasure ecg.decode_batch per
       dirty stripe with both blocks GIVEN (the locate cannot name them: its verdict is MULTIPLE);
  e  one block of every dirty stripe garbage and named, a 4 KiB run in another block:
       heal2_target, and heal_target: the heal's TARGET mode over the same damage (it restores the garbage block
       everywhere but under the run, and leaves the run: its time is the comparison, not its result).
Every case prints ONE JSON line -- bytes read, median / min / max ms and the fraction of 8 TB/s per leg, the ratios
heal2 / heal per round (median, min, max) and the control's -- which the driver appends to --out.  A case asserts the
reports, that the stripes are the encoded ones again after every leg that repairs them, and that
ecg_heal2.counters() moved by S_sel * B * 14 bytes per call.  Needs the GPU: there is no CPU path.

    python tools/heal2_rate.py [--stripes 4096] [--dirty-every 8] [--block 1048576] [--rounds 20] [--warmup 3]
                               [--cases acde] [--out profiles/heal2/heal2_rate.jsonl] [--limit 420] [--rotate 0]
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
RUN = 4096     # damaged bytes per run
LEGS = {"a": ("heal_any", "heal2_any", "heal_any_c1", "heal_any_c2"),
        "c": ("heal_any", "heal2_any", "heal_any_c1", "heal_any_c2"),
        "d": ("heal2_any", "locate_decode2"),
        "e": ("heal2_target", "heal_target")}


def run_case(args, case):
    import torch

    import ecg
    import ecg_heal
    import ecg_heal2
    import ecg_locate

    if not torch.cuda.is_available():
        sys.exit("heal2_rate.py needs an MI355X (torch.cuda.is_available() is False)")
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
    first = torch.arange(D, device="cuda") % k               # the (first) damaged data block of dirty stripe i
    second = (first + 3) % k                                 # cases d, e: the other one
    targets = first.to(torch.int32).contiguous()
    host_rows, host_first, host_second = rows.cpu().tolist(), first.cpu().tolist(), second.cpu().tolist()
    lo = (B // 3) & ~15
    clean1, clean2 = stripes[rows, first].clone(), stripes[rows, second].clone()      # [D][B] each, as encoded
    if case == "e":
        garbage = torch.empty((D, B), dtype=torch.uint8, device="cuda")
        ecg.fill_random(garbage, 0xBAD)
    report = torch.empty((D, n + 2), dtype=torch.int32, device="cuda")
    report2 = torch.empty((D, n + 3), dtype=torch.int32, device="cuda")
    votes = torch.empty((D, n + 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def damage():
        if case == "a":
            stripes[rows, first, lo:lo + RUN] = clean1[:, lo:lo + RUN] ^ 0x5A
        elif case == "d":
            stripes[rows, first, lo:lo + RUN] = clean1[:, lo:lo + RUN] ^ 0x5A
            stripes[rows, second, lo:lo + RUN] = clean2[:, lo:lo + RUN] ^ 0xC3
        elif case == "e":
            stripes[rows, first] = garbage
            stripes[rows, second, lo:lo + RUN] = clean2[:, lo:lo + RUN] ^ 0xC3

    def restore():
        stripes[rows, first] = clean1
        stripes[rows, second] = clean2

    def repaired():
        return torch.equal(stripes[rows, first], clean1) and torch.equal(stripes[rows, second], clean2)

    def heal_any():
        ecg_heal.encode_batch(k, m, M, stripes, stripe_ids=sel, out=report)

    def heal_target():
        ecg_heal.encode_batch(k, m, M, stripes, stripe_ids=sel, targets=targets, out=report)

    def heal2_any():
        ecg_heal2.encode_batch(k, m, M, stripes, stripe_ids=sel, out=report2)

    def heal2_target():
        ecg_heal2.encode_batch(k, m, M, stripes, stripe_ids=sel, targets=targets, out=report2)

    def locate_decode2():
        ecg_locate.encode_batch(k, m, M, stripes, stripe_ids=sel, out=votes)
        v = votes.cpu().numpy()
        with ecg.batch():
            for i, s in enumerate(host_rows):
                if v[i, n]:
                    ecg.decode_batch(k, m, M, row_k_ones, [sorted((host_first[i], host_second[i]))], stripes[s:s + 1])

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    def check(name):
        if name.startswith("heal2"):
            r = report2.cpu().numpy()
            pairs, left, bad = r[:, n + 2], r[:, n + 1], r[:, n]
            assert not left.any(), f"{name}: positions left untouched"
            if case in ("a", "c"):
                assert not pairs.any() and (bad == (RUN if case == "a" else 0)).all(), (name, bad[:4])
            elif case == "d":
                assert (pairs == RUN).all() and (bad == RUN).all(), (name, pairs[:4])
            else:
                assert (pairs > 0.98 * RUN).all() and (bad > 0.99 * B).all(), (name, pairs[:4])
            assert repaired(), f"{name}: the stripes are not the encoded ones again"
        elif name.startswith("heal_any"):
            r = report.cpu().numpy()
            assert (r[:, n] == (RUN if case == "a" else 0)).all() and not r[:, n + 1].any(), name
            assert repaired(), f"{name}: the stripes are not the encoded ones again"
        elif name == "locate_decode2":
            assert repaired(), f"{name}: the stripes are not the encoded ones again"
        else:                                                # heal_target in case e: the run's positions stay
            r = report.cpu().numpy()
            assert (r[range(D), host_first] > 0.98 * (B - RUN)).all() and (r[:, n + 1] > 0.98 * RUN).all(), name

    fns = {"heal_any": heal_any, "heal_any_c1": heal_any, "heal_any_c2": heal_any, "heal2_any": heal2_any,
           "heal_target": heal_target, "heal2_target": heal2_target, "locate_decode2": locate_decode2}
    legs = LEGS[case][args.rotate % len(LEGS[case]):] + LEGS[case][:args.rotate % len(LEGS[case])]
    ms = {name: [] for name in legs}
    c0 = None
    calls2 = sum(name.startswith("heal2") for name in legs)
    for rnd in range(args.warmup + args.rounds):
        if rnd == args.warmup:
            torch.cuda.synchronize()
            c0 = ecg_heal2.counters()
        for name in legs:
            damage()
            torch.cuda.synchronize()
            t = timed(fns[name])
            if rnd >= args.warmup:
                ms[name].append(t)
            if rnd in (0, args.warmup + args.rounds - 1):    # outside the timed region
                check(name)
            if name == "heal_target":
                restore()
    c1 = ecg_heal2.counters()
    assert c1["bytes"] - c0["bytes"] == calls2 * args.rounds * D * B * n, (c0, c1)
    assert c1["launches"] - c0["launches"] == calls2 * args.rounds

    out = {"tool": "heal2_rate", "case": case, "leg_order": list(legs), "code": "RS(10,4)", "stripes": S,
           "dirty_stripes": D,
           "block_bytes": B, "rounds": args.rounds, "warmup": args.warmup, "peak_bytes_per_s": PEAK,
           "device": torch.cuda.get_device_name(0)}
    for name, t in ms.items():
        med = statistics.median(t)
        out[name] = {"bytes": D * B * n, "ms": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                     "frac_of_8TBps": round(D * B * n / (med * 1e-3) / PEAK, 4)}

    def ratio(x, y):
        q = [a / b for a, b in zip(ms[x], ms[y])]
        return {"median": round(statistics.median(q), 4), "min": round(min(q), 4), "max": round(max(q), 4),
                "of_medians": round(out[x]["ms"] / out[y]["ms"], 4)}

    if case in ("a", "c"):
        out["heal2_any_over_heal_any"] = ratio("heal2_any", "heal_any")
        out["control_c1_over_heal_any"] = ratio("heal_any_c1", "heal_any")
        out["control_c2_over_c1"] = ratio("heal_any_c2", "heal_any_c1")
    elif case == "d":
        out["heal2_any_over_locate_decode2"] = ratio("heal2_any", "locate_decode2")
    else:
        out["heal2_target_over_heal_target"] = ratio("heal2_target", "heal_target")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--dirty-every", type=int, default=8, help="one stripe in this many is dirty")
    ap.add_argument("--block", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="acde")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heal2", "heal2_rate.jsonl"))
    ap.add_argument("--limit", type=int, default=420, help="seconds a case may take")
    ap.add_argument("--rotate", type=int, default=0, help="start every round with leg number ROTATE of the case")
    ap.add_argument("--case", choices=sorted(LEGS), help="run this one case in this process (the driver's child)")
    args = ap.parse_args()
    if args.case:
        return run_case(args, args.case)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for case in args.cases:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--stripes", str(args.stripes),
               "--dirty-every", str(args.dirty_every), "--block", str(args.block), "--rounds", str(args.rounds),
               "--warmup", str(args.warmup), "--rotate", str(args.rotate)]
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
