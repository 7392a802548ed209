#!/usr/bin/env python3
"""Delta-update rate against the path it replaces, in one process per case: RS(10,4), 1 MiB blocks, 4096 stripes
resident in HBM.

The legs alternate within a round, each timed by HIP events after a warm-up, so box-to-box and minute-to-minute drift
hits them alike:
  update     ecg_update.encode_batch: one launch over the case's records (device-resident), the report reused;
  reencode   what the library offered before: copy the new bytes into place (one indexed copy over a precomputed
             index, or one block copy per call for whole-block records), then re-encode the touched stripes with
             ecg.matrix_apply_batch_multi and stripe_of -- (k + m) * B bytes per touched stripe whatever the change.
Every call gets another of four random staging buffers, so no leg ever writes the bytes that are already there (a
column whose delta is zero is skipped by the update).  Cases:
  a  512 records of 4 KiB, one per stripe, columns and (unaligned) offsets rotating;
  b  512 records of 64 KiB;
  c  512 whole-block records;
  d  8192 records of 4 KiB, 16 per stripe over 512 stripes;
  e  case a in DELTA mode (the update touches the parities only; the comparator is case a's).
The per-record form -- one ecg_matrix_apply_batch over [p_0..p_3, old, new] per record inside a batch scope -- is not
run: a strided call addresses every input as base + id * bstride, and the new bytes live in a staging buffer outside
that pattern, at another offset than the range they replace.
Each case is a fresh child process under its own time limit; the driver stops at the first one that fails.  Every case
prints ONE JSON line -- the bytes by ecg_update_traffic_bytes, median / min / max ms and the fraction of 8 TB/s per
leg, and the update's time over the re-encode's per round -- which the driver appends to --out.  A case asserts that
every record was applied and that all 4096 stripes scrub clean after an update.  Needs the GPU: there is no CPU path.

    python tools/update_rate.py [--stripes 4096] [--block 1048576] [--rounds 20] [--warmup 3] [--cases a,b,c,d,e]
                                [--out profiles/update/update_rate.jsonl] [--limit 420]
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
LEGS = ("update", "reencode")
# case: (records, records per stripe, bytes per record or None = the block, mode)
CASES = {"a": (512, 1, 4096, 0), "b": (512, 1, 65536, 0), "c": (512, 1, None, 0), "d": (8192, 16, 4096, 0),
         "e": (512, 1, 4096, 1)}


def run_case(args, case):
    import numpy as np
    import torch

    import ecg
    import ecg_scrub
    import ecg_update

    if not torch.cuda.is_available():
        sys.exit("update_rate.py needs an MI355X (torch.cuda.is_available() is False)")
    torch.cuda.set_device(0)
    R, per, ln, mode = CASES[case]
    k, m, S, B = 10, 4, args.stripes, args.block
    n = k + m
    ln = B if ln is None else ln
    M = ecg.reed_sol_vandermonde_coding_matrix(k, m)
    stripes = torch.empty((S, n, B), dtype=torch.uint8, device="cuda")
    ecg.fill_random(stripes, 0x0DA7)
    ecg.encode_batch(k, m, M, stripes[:, :k], stripes[:, k:])
    T = R // per                                                     # touched stripes, evenly spread
    recs = np.zeros((R, 5), np.int64)
    for i in range(R):
        t, j = divmod(i, per)
        recs[i] = [t * (S // T) + (S // T) // 2, (t + 3 * j) % k,
                   0 if ln == B else (j * (B // per) + (i * 66067) % (B // per - ln)), ln, i * ln]
    in_bytes = R * ln
    assert ecg_update.check_records(recs, k, B, S, ln, in_bytes, False) == -1
    d_recs = torch.from_numpy(recs).cuda()
    bufs = []
    for q in range(4):
        b = torch.empty((in_bytes,), dtype=torch.uint8, device="cuda")
        ecg.fill_random(b, 0xB0F + q)
        bufs.append(b)
    touched = ecg_update.touched_stripes(recs)
    assert int(touched.numel()) == T
    report = torch.empty((R, 2), dtype=torch.int32, device="cuda")
    prog = ecg.Programs([(M, list(range(k)), list(range(k, n)))])
    rows = torch.from_numpy(recs[:, 0]).cuda()
    cols = torch.from_numpy(recs[:, 1]).cuda()
    if ln == B:
        index = None
    else:                                                            # flat byte index of every record byte
        start = torch.from_numpy((recs[:, 0] * n + recs[:, 1]) * B + recs[:, 2]).cuda()
        index = (start[:, None] + torch.arange(ln, device="cuda")[None, :]).reshape(-1)
    flat = stripes.view(-1)
    calls = [0]
    torch.cuda.synchronize()

    def update():
        calls[0] += 1
        ecg_update.encode_batch(k, m, M, stripes, d_recs, bufs[calls[0] % 4], mode=mode, max_len=ln, out=report)

    def reencode():
        calls[0] += 1
        new = bufs[calls[0] % 4]
        if index is None:
            stripes[rows, cols] = new.view(R, B)
        else:
            flat[index] = new
        ecg.matrix_apply_batch_multi(prog, stripes, stripes, stripe_of=touched)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    legs = {"update": update, "reencode": reencode}
    ms = {name: [] for name in LEGS}
    c0 = None
    for rnd in range(args.warmup + args.rounds):
        if rnd == args.warmup:
            torch.cuda.synchronize()
            c0 = ecg_update.counters()
        for name in LEGS:
            t = timed(legs[name])
            if rnd >= args.warmup:
                ms[name].append(t)
            if name == "update" and rnd in (0, args.warmup + args.rounds - 1):      # outside the timed region
                r = report.cpu().numpy()
                assert not r[:, 0].any(), "a record was refused"
                assert (r[:, 1] > 0.99 * ln).all(), "a record changed fewer bytes than random data would"
    c1 = ecg_update.counters()
    assert c1["launches"] - c0["launches"] == args.rounds and c1["records"] - c0["records"] == args.rounds * R
    calls[0] = 1
    update()                                                         # the stripes are codewords (after a re-encode):
    if mode == 1:                                                    # one update leaves them so; in DELTA mode, the
        calls[0] = 1                                                 # same delta twice
        update()
    bad = ecg_scrub.encode_batch(k, m, M, stripes)
    torch.cuda.synchronize()
    assert not bad.any().item(), "the stripes do not scrub clean after an update"

    nnz = ecg_update.nnz_per_col(M, k)
    moved = {"update": ecg_update.traffic_bytes(nnz, recs, mode, False), "reencode": 2 * in_bytes + T * n * B}
    out = {"tool": "update_rate", "case": case, "mode": "DELTA" if mode else "WRITE", "code": "RS(10,4)", "stripes": S,
           "block_bytes": B, "records": R, "record_bytes": ln, "touched_stripes": T, "rounds": args.rounds,
           "warmup": args.warmup, "peak_bytes_per_s": PEAK, "last_launch": ecg_update.last_launch(),
           "device": torch.cuda.get_device_name(0)}
    for name, t in ms.items():
        med = statistics.median(t)
        out[name] = {"bytes": moved[name], "ms": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                     "frac_of_8TBps": round(moved[name] / (med * 1e-3) / PEAK, 4) if med > 0 else 0.0}
    ratios = [u / r for u, r in zip(ms["update"], ms["reencode"])]
    out["update_time_over_reencode"] = {"median": round(statistics.median(ratios), 4), "min": round(min(ratios), 4),
                                        "max": round(max(ratios), 4)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--block", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="a,b,c,d,e")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update", "update_rate.jsonl"))
    ap.add_argument("--limit", type=int, default=420, help="seconds a case may take")
    ap.add_argument("--case", choices=sorted(CASES), help="run this one case in this process (the driver's child)")
    args = ap.parse_args()
    if args.case:
        return run_case(args, args.case)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for case in args.cases.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--stripes", str(args.stripes), "--block",
               str(args.block), "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
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
