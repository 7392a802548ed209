#!/usr/bin/env python3
"""Degraded-range-read rate against the path it replaces, in one process per case: 1 MiB blocks, 4096 stripes resident
in HBM, 512 of them degraded with one lost data block that rotates per stripe.

The legs alternate within a round, each timed by HIP events after a warm-up, so box-to-box and minute-to-minute drift
hits them alike:
  dread    ecg_dread.encode_batch: the plan launch and the main launch over the case's records (device-resident),
           scratch, answer buffer and report reused;
  decode   what the library offered before: ecg.decode_batch of the 512 degraded stripes (a strided view of the
           store, one single-erasure pattern per lost column) into a scratch of whole blocks, then the copy of the
           asked ranges out of the scratch (one indexed copy over a precomputed index; one copy for whole blocks).
Cases:
  a  512 records of 4 KiB, one per degraded stripe, at unaligned offsets;
  b  512 records of 64 KiB;
  c  8192 records of 4 KiB, 16 per degraded stripe;
  d  512 whole-block records;
  e  Azure(12,2,2), 512 records of 4 KiB: the dread reads the 6 blocks of the local group, the decode the class's k.
Each case is a fresh child process under its own time limit; the driver stops at the first one that fails.  Every case
prints ONE JSON line -- the bytes by the definition (reads * len read and len written per record; the decode's
(k + 1) * B per stripe and the copy's 2 * len), median / min / max ms and the fraction of 8 TB/s per leg, and the
dread's time over the decode's per round -- which the driver appends to --out.  A case asserts that every record was
answered with the reads the plan rule gives and that both legs return the bytes the lost blocks held.  Needs the GPU:
there is no CPU path.

    python tools/dread_rate.py [--stripes 4096] [--block 1048576] [--rounds 20] [--warmup 3] [--cases a,b,c,d,e]
                               [--out profiles/dread/dread_rate.jsonl] [--limit 420]
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
LEGS = ("dread", "decode")
DEGRADED = 512
# case: (code, records, records per stripe, bytes per record or None = the block)
CASES = {"a": ("RS(10,4)", 512, 1, 4096), "b": ("RS(10,4)", 512, 1, 65536), "c": ("RS(10,4)", 8192, 16, 4096),
         "d": ("RS(10,4)", 512, 1, None), "e": ("Azure(12,2,2)", 512, 1, 4096)}


def run_case(args, case):
    import numpy as np
    import torch

    import ecg
    import ecg_dread

    if not torch.cuda.is_available():
        sys.exit("dread_rate.py needs an MI355X (torch.cuda.is_available() is False)")
    torch.cuda.set_device(0)
    name, R, per, ln = CASES[case]
    S, B, T = args.stripes, args.block, DEGRADED
    if name == "RS(10,4)":
        k, m = 10, 4
        M = ecg.reed_sol_vandermonde_coding_matrix(k, m)
        want_reads = k
    else:
        k, m = 12, 4
        M = ecg.ec_factory(ecg.ECTYPE.AZURE_LRC, ecg.CodingParameters(k=12, l=2, g=2)).make_encoding_matrix()
        want_reads = k // 2                                          # the local group: 5 data blocks and its parity
    n = k + m
    ln = B if ln is None else ln
    assert S % T == 0 and R == T * per
    step, first = S // T, (S // T) // 2                              # degraded stripe t is stripe first + t * step
    stripes = torch.empty((S, n, B), dtype=torch.uint8, device="cuda")
    ecg.fill_random(stripes, 0x0D2EAD)
    ecg.encode_batch(k, m, M, stripes[:, :k], stripes[:, k:])
    lost_col = np.arange(T) % k
    recs = np.zeros((R, 5), np.int64)
    for i in range(R):
        t, j = divmod(i, per)
        off = 0 if ln == B else (j * (B // per) + (i * 66067) % (B // per - ln))
        recs[i] = [first + t * step, lost_col[t], off, ln, i * ln]
    out_bytes = R * ln
    assert ecg_dread.check_records(recs, n, B, S, ln, out_bytes) == -1
    if ln != B:
        assert (recs[:, 2] % 16 != 0).any()
    rows = torch.from_numpy(recs[:, 0]).cuda()
    cols = torch.from_numpy(recs[:, 1]).cuda()
    if ln == B:
        index = None
        truth = stripes[rows, cols].reshape(-1).clone()
    else:                                                            # byte index of every record byte in the scratch
        start = torch.from_numpy((recs[:, 0] - first) // step * B + recs[:, 2]).cuda()
        index = (start[:, None] + torch.arange(ln, device="cuda")[None, :]).reshape(-1)
        src = torch.from_numpy((recs[:, 0] * n + recs[:, 1]) * B + recs[:, 2]).cuda()
        truth = stripes.view(-1)[(src[:, None] + torch.arange(ln, device="cuda")[None, :]).reshape(-1)]
    lost = np.zeros((S, n), np.uint8)
    lost[first + np.arange(T) * step, lost_col] = 1
    stripes[torch.from_numpy(first + np.arange(T) * step).cuda(), torch.from_numpy(lost_col).cuda()] = 0xA5
    d_lost = torch.from_numpy(lost).cuda()
    d_recs = torch.from_numpy(recs).cuda()
    out = torch.empty((out_bytes,), dtype=torch.uint8, device="cuda")
    alt = torch.empty((out_bytes,), dtype=torch.uint8, device="cuda")
    work = torch.empty((ecg_dread.work_bytes(R, n),), dtype=torch.uint8, device="cuda")
    report = torch.empty((R, 2), dtype=torch.int32, device="cuda")
    degraded = stripes[first::step]                                  # [T][n][B], a strided view of the store
    assert degraded.shape[0] == T
    scratch = torch.empty((T, 1, B), dtype=torch.uint8, device="cuda")
    patterns = [[e] for e in range(k)]
    pos = torch.from_numpy(lost_col.astype(np.int32)).cuda()
    torch.cuda.synchronize()

    def dread():
        ecg_dread.encode_batch(k, m, M, stripes, d_lost, d_recs, out, max_len=ln, work=work, report=report)

    def decode():
        ecg.decode_batch(k, m, M, 0, patterns, degraded, out=scratch, pattern_of_stripe=pos)
        if index is None:
            alt.copy_(scratch.view(-1))
        else:
            torch.index_select(scratch.view(-1), 0, index, out=alt)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    legs = {"dread": dread, "decode": decode}
    ms = {leg: [] for leg in LEGS}
    c0 = None
    for rnd in range(args.warmup + args.rounds):
        if rnd == args.warmup:
            torch.cuda.synchronize()
            c0 = ecg_dread.counters()
        for leg in LEGS:
            t = timed(legs[leg])
            if rnd >= args.warmup:
                ms[leg].append(t)
        if rnd in (0, args.warmup + args.rounds - 1):                # outside the timed region
            r = report.cpu().numpy()
            assert not r[:, 0].any(), "a record was refused"
            assert (r[:, 1] == want_reads).all(), f"reads {sorted(set(r[:, 1].tolist()))}, not {want_reads}"
            assert torch.equal(out, truth), "the dread's answer is not what the lost blocks held"
            assert torch.equal(alt, truth), "the decode's answer is not what the lost blocks held"
            out.fill_(0)
            alt.fill_(0)
    c1 = ecg_dread.counters()
    assert c1["launches"] - c0["launches"] == args.rounds and c1["records"] - c0["records"] == args.rounds * R

    moved = {"dread": R * ln * (want_reads + 1), "decode": T * (k + 1) * B + 2 * R * ln}
    res = {"tool": "dread_rate", "case": case, "code": name, "stripes": S, "block_bytes": B, "degraded_stripes": T,
           "records": R, "record_bytes": ln, "reads_per_record": want_reads, "rounds": args.rounds,
           "warmup": args.warmup, "peak_bytes_per_s": PEAK, "last_launch": ecg_dread.last_launch(),
           "device": torch.cuda.get_device_name(0)}
    for leg, t in ms.items():
        med = statistics.median(t)
        res[leg] = {"bytes": moved[leg], "ms": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                    "frac_of_8TBps": round(moved[leg] / (med * 1e-3) / PEAK, 4) if med > 0 else 0.0}
    ratios = [a / b for a, b in zip(ms["dread"], ms["decode"])]
    res["dread_time_over_decode"] = {"median": round(statistics.median(ratios), 4), "min": round(min(ratios), 4),
                                     "max": round(max(ratios), 4)}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--block", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="a,b,c,d,e")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dread", "dread_rate.jsonl"))
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
