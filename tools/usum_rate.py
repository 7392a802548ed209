#!/usr/bin/env python3
"""Update-sum rate against the path it replaces, in one process per case: RS(10,4), 1 MiB blocks, 4096 stripes
resident in HBM, 512 of them touched (the store of tools/update_rate.py, whose cases a-d these are).

The legs alternate within a round, each timed by HIP events after a warm-up, so box-to-box and minute-to-minute drift
hits them alike:
  update         ecg_update.encode_batch in WRITE mode with its delta output: what a store without sums pays;
  usum           ecg_usum.apply alone, over the delta and the report the update left;
  update_usum    the update, then ecg_usum.apply into the store's sum table: the cheap write path with sums kept;
  update_resum   what the library offered before: the update, then ecg_sum.blocks_batch (piece_bytes 0) or
                 ecg_psum.pieces_batch over ecg_update.touched_stripes -- n * B bytes per touched stripe.
Every call gets another of four random staging buffers, so no update writes the bytes that are already there.  Cases:
  a  512 records of 4 KiB, one per stripe, columns and (unaligned) offsets rotating;
  b  512 records of 64 KiB;
  c  512 whole-block records;
  d  8192 records of 4 KiB, 16 per stripe over 512 stripes;
each at piece_bytes 0 (one sum per block) and 4096.  Each (case, piece_bytes) is a fresh child process under its own
time limit; the driver stops at the first one that fails.  Every case prints ONE JSON line -- median / min / max ms per
leg, update_usum over update_resum and over update per round -- which the driver appends to --out.  A case asserts
that every record was applied and, after the timed rounds, that the table one update + usum leaves for the touched
stripes equals their fresh sums.  Needs the GPU: there is no CPU path.

    python tools/usum_rate.py [--stripes 4096] [--block 1048576] [--rounds 20] [--warmup 3] [--cases a,b,c,d]
                              [--pieces 0,4096] [--out profiles/usum/usum_rate.jsonl] [--limit 420]
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

LEGS = ("update", "usum", "update_usum", "update_resum")
# case: (records, records per stripe, bytes per record or None = the block)
CASES = {"a": (512, 1, 4096), "b": (512, 1, 65536), "c": (512, 1, None), "d": (8192, 16, 4096)}


def run_case(args, case, piece_bytes):
    import numpy as np
    import torch

    import ecg
    import ecg_psum
    import ecg_sum
    import ecg_update
    import ecg_usum

    if not torch.cuda.is_available():
        sys.exit("usum_rate.py needs an MI355X (torch.cuda.is_available() is False)")
    torch.cuda.set_device(0)
    R, per, ln = CASES[case]
    k, m, S, B = 10, 4, args.stripes, args.block
    n = k + m
    ln = B if ln is None else ln
    Q = ecg_usum.pieces(B, piece_bytes)
    M = ecg.reed_sol_vandermonde_coding_matrix(k, m)
    ids = list(range(n))
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
    assert ecg_update.check_records(recs, k, B, S, ln, in_bytes, True) == -1
    d_recs = torch.from_numpy(recs).cuda()
    bufs = []
    for q in range(4):
        b = torch.empty((in_bytes,), dtype=torch.uint8, device="cuda")
        ecg.fill_random(b, 0xB0F + q)
        bufs.append(b)
    delta = torch.zeros((in_bytes,), dtype=torch.uint8, device="cuda")
    touched = ecg_update.touched_stripes(recs)
    assert int(touched.numel()) == T
    report = torch.empty((R, 2), dtype=torch.int32, device="cuda")
    report2 = torch.empty((R, 2), dtype=torch.int32, device="cuda")
    fresh = torch.empty((T, n, Q), dtype=torch.int32, device="cuda")

    def sums_of(stripe_ids, out=None):
        if piece_bytes == 0:
            v = ecg_sum.blocks_batch(ids, stripes, stripe_ids=stripe_ids, out=None if out is None else out.view(-1, n))
            return v.view(-1, n, 1)
        return ecg_psum.pieces_batch(ids, stripes, piece_bytes, stripe_ids=stripe_ids, out=out)

    table = sums_of(None).contiguous()                               # the store's recorded table, all S stripes
    calls = [0]
    torch.cuda.synchronize()

    def update():
        calls[0] += 1
        ecg_update.encode_batch(k, m, M, stripes, d_recs, bufs[calls[0] % 4], max_len=ln, delta_out=delta, out=report)

    def usum():
        ecg_usum.apply(table, d_recs, delta, B, k=k, m=m, matrix=M, piece_bytes=piece_bytes, max_len=ln,
                       update_report=report, out=report2)

    def update_usum():
        update()
        usum()

    def update_resum():
        update()
        sums_of(touched, fresh)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    legs = {"update": update, "usum": usum, "update_usum": update_usum, "update_resum": update_resum}
    ms = {name: [] for name in LEGS}
    for rnd in range(args.warmup + args.rounds):
        for name in LEGS:
            t = timed(legs[name])
            if rnd >= args.warmup:
                ms[name].append(t)
            if name == "update_usum" and rnd in (0, args.warmup + args.rounds - 1):     # outside the timed region
                r, r2 = report.cpu().numpy(), report2.cpu().numpy()
                assert not r[:, 0].any() and not r2[:, 0].any(), "a record was refused"
                assert (r[:, 1] > 0.99 * ln).all() and (r == r2).all(), "the two reports differ"
    # the table is the update's sums: from fresh sums of the touched stripes, one update and one usum
    sums_of(touched, fresh)
    table[touched.long()] = fresh
    update_usum()
    sums_of(touched, fresh)
    torch.cuda.synchronize()
    assert torch.equal(table[touched.long()], fresh), "update + usum does not leave the sums of the stripes"

    nnz = ecg_update.nnz_per_col(M, k)
    out = {"tool": "usum_rate", "case": case, "piece_bytes": piece_bytes, "code": "RS(10,4)", "stripes": S,
           "block_bytes": B, "records": R, "record_bytes": ln, "touched_stripes": T, "rounds": args.rounds,
           "warmup": args.warmup, "last_launch": ecg_usum.last_launch(),
           "bytes": {"update": ecg_update.traffic_bytes(nnz, recs, 0, True),
                     "usum": ecg_usum.traffic_bytes(nnz, recs, B, piece_bytes), "resum": T * n * B},
           "device": torch.cuda.get_device_name(0)}
    for name, t in ms.items():
        out[name] = {"ms": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4)}
    for key, other in (("update_usum_over_update_resum", "update_resum"), ("update_usum_over_update", "update")):
        ratios = [u / r for u, r in zip(ms["update_usum"], ms[other])]
        out[key] = {"median": round(statistics.median(ratios), 4), "min": round(min(ratios), 4),
                    "max": round(max(ratios), 4)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--block", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="a,b,c,d")
    ap.add_argument("--pieces", default="0,4096")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "usum", "usum_rate.jsonl"))
    ap.add_argument("--limit", type=int, default=420, help="seconds a case may take")
    ap.add_argument("--case", choices=sorted(CASES), help="run this one case in this process (the driver's child)")
    ap.add_argument("--piece", type=int, default=0, help="piece_bytes of --case")
    args = ap.parse_args()
    if args.case:
        return run_case(args, args.case, args.piece)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for case in args.cases.split(","):
        for piece in args.pieces.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--piece", piece, "--stripes",
                   str(args.stripes), "--block", str(args.block), "--rounds", str(args.rounds), "--warmup",
                   str(args.warmup)]
            try:
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                sys.exit(f"case {case} piece_bytes {piece} did not finish in {args.limit} s: stopping")
            if res.returncode != 0:
                sys.stderr.write(res.stdout + res.stderr)
                sys.exit(f"case {case} piece_bytes {piece} failed with status {res.returncode}: stopping")
            line = res.stdout.strip().splitlines()[-1]
            json.loads(line)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
