#!/usr/bin/env python3
"""Locate rate against the scrub, in one process per case: RS(10,4), 1 MiB blocks, the dirty subset of 4096 stripes
resident in HBM.

The locate (ecg_locate.encode_batch with stripe_ids = the dirty stripes) runs over the big array through its
selection; the yardstick is the same run's ecg_scrub.encode_batch over a contiguous copy of the same dirty stripes
(the scrub has no selection).  Both are timed by HIP events after a warm-up and alternate within a round, so
box-to-box and minute-to-minute drift hits them alike.  Cases:
  a  one 4 KiB run damaged in one data block of every dirty stripe (what a torn sector looks like);
  b  one whole data block of every dirty stripe replaced by garbage (every column runs the candidate test);
  c  the same selection over all-clean stripes (the locate's floor: the clean fast path everywhere).
Each case is a fresh child process under its own time limit; the driver stops at the first one that fails.  Every
case prints ONE JSON line -- bytes read, median / min / max ms and the fraction of 8 TB/s for both legs, and the
locate's time over the scrub's -- which the driver appends to --out.  A case asserts its votes (every dirty stripe
names its block, with 4096 / nearly B / no bad positions) and that ecg_locate.counters() moved by S_sel * B * 14
bytes per locate.  Needs the GPU: there is no CPU path.

    python tools/locate_rate.py [--stripes 4096] [--dirty-every 8] [--block 1048576] [--rounds 20] [--warmup 3]
                                [--cases abc] [--out profiles/locate/locate_rate.jsonl] [--limit 240]
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
BLOCK = 3      # the damaged data block


def run_case(args, case):
    import torch

    import ecg
    import ecg_locate
    import ecg_scrub

    if not torch.cuda.is_available():
        sys.exit("locate_rate.py needs an MI355X (torch.cuda.is_available() is False)")
    torch.cuda.set_device(0)
    k, m, S, B = 10, 4, args.stripes, args.block
    n = k + m
    M = ecg.reed_sol_vandermonde_coding_matrix(k, m)
    stripes = torch.empty((S, n, B), dtype=torch.uint8, device="cuda")
    ecg.fill_random(stripes, 0x10CA7E)
    ecg.encode_batch(k, m, M, stripes[:, :k], stripes[:, k:])
    sel = torch.arange(args.dirty_every // 2, S, args.dirty_every, dtype=torch.int32, device="cuda")
    D = int(sel.numel())
    rows = sel.long()
    if case == "a":
        lo = (B // 3) & ~15
        stripes[rows, BLOCK, lo:lo + RUN] ^= 0x5A
    elif case == "b":
        garbage = torch.empty((D, 1, B), dtype=torch.uint8, device="cuda")
        ecg.fill_random(garbage, 0xBAD)
        stripes[rows, BLOCK] = garbage[:, 0]
        del garbage
    packed = stripes[rows].contiguous()  # the scrub leg's copy of the dirty stripes
    votes = torch.empty((D, n + 2), dtype=torch.int32, device="cuda")
    counts = torch.empty((D, m), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def locate():
        ecg_locate.encode_batch(k, m, M, stripes, stripe_ids=sel, out=votes)

    def scrub():
        ecg_scrub.encode_batch(k, m, M, packed, out=counts)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    ms = {"locate": [], "scrub": []}
    for _ in range(args.warmup):
        locate(), scrub()
    torch.cuda.synchronize()
    c0 = ecg_locate.counters()
    for _ in range(args.rounds):
        ms["locate"].append(timed(locate))
        ms["scrub"].append(timed(scrub))
    c1 = ecg_locate.counters()
    assert c1["bytes"] - c0["bytes"] == args.rounds * D * B * n, (c0, c1)
    assert c1["launches"] - c0["launches"] == args.rounds

    v = votes.cpu().numpy()
    dirty_rows = (counts != 0).any(dim=1).sum().item()
    if case == "c":
        assert not v.any() and dirty_rows == 0, "clean stripes reported a vote"
    else:
        assert dirty_rows == D
        bad = v[:, n]
        assert (v[:, BLOCK] == bad).all() and not v[:, n + 1].any(), "a dirty stripe does not name its block"
        assert not v[:, [b for b in range(n) if b != BLOCK]].any()
        assert (bad == RUN).all() if case == "a" else (bad > 0.99 * B).all(), bad[:4]
        assert all(ecg_locate.verdict(row) == (BLOCK, [BLOCK]) for row in v[:8])

    out = {"tool": "locate_rate", "case": case, "code": "RS(10,4)", "stripes": S, "dirty_stripes": D,
           "block_bytes": B, "rounds": args.rounds, "warmup": args.warmup, "peak_bytes_per_s": PEAK,
           "device": torch.cuda.get_device_name(0)}
    for name, t in ms.items():
        med = statistics.median(t)
        out[name] = {"bytes": D * B * n, "ms": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                     "frac_of_8TBps": round(D * B * n / (med * 1e-3) / PEAK, 4)}
    out["locate_time_over_scrub"] = round(out["locate"]["ms"] / out["scrub"]["ms"], 4)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--dirty-every", type=int, default=8, help="one stripe in this many is dirty")
    ap.add_argument("--block", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="abc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate", "locate_rate.jsonl"))
    ap.add_argument("--limit", type=int, default=240, help="seconds a case may take")
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
