#!/usr/bin/env python3
"""Verified-range-read rate against the two things it is weighed against, in one process per case: the store, rounds and
interleaving of tools/dread_rate.py -- 1 MiB blocks, 4096 RS(10,4) stripes resident in HBM, 512 of them degraded with
one lost data block that rotates per stripe.

The legs alternate within a round, each timed by HIP events after a warm-up, so box-to-box and minute-to-minute drift
hits them alike:
  vread     ecg_vread.encode_batch: the plan launch, the main launch and the verdict launch over the case's records
            (device-resident), scratch, answer buffer, sums and report reused;
  dread     (a) the unverified ecg_dread.encode_batch of the same records: the price of verification;
  composed  (b) what a verified read cost before: ecg_dread of the covering pieces into a scratch, ecg_psum.pieces_batch
            over the scratch viewed as P-byte blocks, the compare with the recorded sums (gathered per record before
            the timed region) and the copy of the asked ranges out of the scratch (one indexed copy over a precomputed
            index; one copy for whole blocks).
Cases (512 records, one per degraded stripe; "u" = the range straddles a piece boundary):
  a, au   4 KiB at P = 4 KiB, piece-aligned / two pieces covered      <- the gate: vread / composed < 1 (median)
  b, bu   4 KiB at P = 512, 8 / 9 pieces covered
  c, cu   4 KiB at P = 64 KiB, one / two pieces covered
  d       64 KiB at P = 4 KiB, 17 pieces covered
  e       whole blocks with block sums
Each case is a fresh child process under its own time limit; the driver stops at the first one that fails and exits 1
if a gated case misses the gate.  Every case prints ONE JSON line -- the bytes by the definition (vread: reads * cover
read and len written per record), median / min / max ms per leg and the vread's time over either comparison per round
-- which the driver appends to --out.  A case asserts that every record was answered in state 0 with the reads the
plan rule gives, that the composed leg finds no bad piece and that all three legs return the bytes the lost blocks
held.  Needs the GPU: there is no CPU path.

    python tools/vread_rate.py [--stripes 4096] [--block 1048576] [--rounds 20] [--warmup 3]
                               [--cases a,au,b,bu,c,cu,d,e] [--out profiles/vread/vread_rate.jsonl] [--limit 420]
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
LEGS = ("vread", "dread", "composed")
DEGRADED = 512
# case: (bytes per record or None = the block, piece_bytes, straddling, gated)
CASES = {"a": (4096, 4096, False, True), "au": (4096, 4096, True, True), "b": (4096, 512, False, False),
         "bu": (4096, 512, True, False), "c": (4096, 65536, False, False), "cu": (4096, 65536, True, False),
         "d": (65536, 4096, True, False), "e": (None, 0, False, False)}


def run_case(args, case):
    import numpy as np
    import torch

    import ecg
    import ecg_dread
    import ecg_psum
    import ecg_vread

    if not torch.cuda.is_available():
        sys.exit("vread_rate.py needs an MI355X (torch.cuda.is_available() is False)")
    torch.cuda.set_device(0)
    ln, P, straddle, gated = CASES[case]
    S, B, R = args.stripes, args.block, DEGRADED
    k, m = 10, 4
    n = k + m
    M = ecg.reed_sol_vandermonde_coding_matrix(k, m)
    ln = B if ln is None else ln
    Pk = P or B                                                      # block sums: the block is the one piece
    assert S % R == 0 and B % Pk == 0 and ln <= B
    step, first = S // R, (S // R) // 2                              # degraded stripe t is stripe first + t * step
    stripes = torch.empty((S, n, B), dtype=torch.uint8, device="cuda")
    ecg.fill_random(stripes, 0x0D2EAD)
    ecg.encode_batch(k, m, M, stripes[:, :k], stripes[:, k:])
    expected = ecg_psum.pieces_batch(list(range(n)), stripes, Pk)   # the recorded table, before anything is lost
    Q = B // Pk
    lost_col = np.arange(R) % k
    shift = 0 if not straddle else (Pk - ln // 2 - 3 if ln <= Pk else 5)
    npieces = -(-(shift + ln) // Pk)
    cover = npieces * Pk
    recs = np.zeros((R, 5), np.int64)
    crecs = np.zeros((R, 5), np.int64)                               # the covers, for the composed leg
    for i in range(R):
        q0 = 0 if ln == B else (i * 66067) % (Q - npieces)           # away from the block's last piece
        recs[i] = [first + i * step, lost_col[i], q0 * Pk + shift, ln, i * ln]
        crecs[i] = [first + i * step, lost_col[i], q0 * Pk, cover, i * cover]
    out_bytes = R * ln
    assert ecg_vread.check_records(recs, n, B, S, ln, out_bytes) == -1
    assert all(ecg_vread.cover(int(r[2]), ln, P, B) == (int(r[2]) // Pk, npieces, cover) for r in recs[:8])
    ar = torch.arange(ln, device="cuda")[None, :]
    src = torch.from_numpy((recs[:, 0] * n + recs[:, 1]) * B + recs[:, 2]).cuda()
    truth = stripes.view(-1)[(src[:, None] + ar).reshape(-1)]
    index = None if ln == cover else (torch.from_numpy(np.arange(R) * cover + shift).cuda()[:, None] + ar).reshape(-1)
    rows = torch.from_numpy((recs[:, 0] * n + recs[:, 1]) * Q + recs[:, 2] // Pk).cuda()
    want_sums = expected.view(-1)[(rows[:, None] + torch.arange(npieces, device="cuda")[None, :])]   # (R, npieces)
    lost = np.zeros((S, n), np.uint8)
    lost[recs[:, 0], lost_col] = 1
    stripes[torch.from_numpy(recs[:, 0]).cuda(), torch.from_numpy(lost_col).cuda()] = 0xA5
    d_lost = torch.from_numpy(lost).cuda()
    d_recs, d_crecs = torch.from_numpy(recs).cuda(), torch.from_numpy(crecs).cuda()
    out, alt, plain = (torch.empty((out_bytes,), dtype=torch.uint8, device="cuda") for _ in range(3))
    work = torch.empty((ecg_vread.work_bytes(R, n),), dtype=torch.uint8, device="cuda")
    NP = ecg_vread.max_pieces(ln, P, B)
    report = torch.empty((R, 4), dtype=torch.int32, device="cuda")
    sums = torch.empty((R, NP), dtype=torch.int32, device="cuda")
    dreport, creport = (torch.empty((R, 2), dtype=torch.int32, device="cuda") for _ in range(2))
    scratch = torch.empty((R, npieces, Pk), dtype=torch.uint8, device="cuda")
    csums = torch.empty((R, npieces, 1), dtype=torch.int32, device="cuda")
    pieces = list(range(npieces))
    bad = torch.zeros((R,), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def vread():
        ecg_vread.encode_batch(k, m, M, stripes, d_lost, P, expected, d_recs, out, max_len=ln, work=work, report=report,
                               sums=sums)

    def dread():
        ecg_dread.encode_batch(k, m, M, stripes, d_lost, d_recs, plain, max_len=ln, work=work, report=dreport)

    def composed():
        ecg_dread.encode_batch(k, m, M, stripes, d_lost, d_crecs, scratch.view(-1), max_len=cover, work=work,
                               report=creport)
        ecg_psum.pieces_batch(pieces, scratch, Pk, out=csums)
        torch.sum(csums.view(R, npieces) != want_sums, dim=1, out=bad)
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

    legs = {"vread": vread, "dread": dread, "composed": composed}
    ms = {leg: [] for leg in LEGS}
    c0 = None
    for rnd in range(args.warmup + args.rounds):
        if rnd == args.warmup:
            torch.cuda.synchronize()
            c0 = ecg_vread.counters()
        for leg in LEGS:
            t = timed(legs[leg])
            if rnd >= args.warmup:
                ms[leg].append(t)
        if rnd in (0, args.warmup + args.rounds - 1):                # outside the timed region
            r = report.cpu().numpy()
            assert not r[:, 0].any() and not r[:, 2].any(), f"states {sorted(set(r[:, 0].tolist()))}"
            assert (r[:, 1] == k).all(), f"reads {sorted(set(r[:, 1].tolist()))}, not {k}"
            assert torch.equal(sums[:, :npieces], want_sums), "the vread's sums are not the recorded ones"
            assert not dreport[:, 0].any().item() and not creport[:, 0].any().item() and not bad.any().item()
            for name, buf in (("vread", out), ("dread", plain), ("composed", alt)):
                assert torch.equal(buf, truth), f"the {name}'s answer is not what the lost blocks held"
                buf.fill_(0)
    c1 = ecg_vread.counters()
    assert c1["launches"] - c0["launches"] == args.rounds and c1["records"] - c0["records"] == args.rounds * R

    moved = {"vread": R * (k * cover + ln), "dread": R * ln * (k + 1),
             "composed": R * ((k + 1) * cover + cover + 2 * ln)}
    res = {"tool": "vread_rate", "case": case, "code": "RS(10,4)", "stripes": S, "block_bytes": B,
           "degraded_stripes": R, "records": R, "record_bytes": ln, "piece_bytes": P, "pieces_per_record": npieces,
           "cover_bytes": cover, "reads_per_record": k, "rounds": args.rounds, "warmup": args.warmup,
           "peak_bytes_per_s": PEAK, "last_launch": ecg_vread.last_launch(), "device": torch.cuda.get_device_name(0)}
    for leg, t in ms.items():
        med = statistics.median(t)
        res[leg] = {"bytes": moved[leg], "ms": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                    "frac_of_8TBps": round(moved[leg] / (med * 1e-3) / PEAK, 4) if med > 0 else 0.0}
    for other in ("dread", "composed"):
        ratios = [a / b for a, b in zip(ms["vread"], ms[other])]
        res[f"vread_time_over_{other}"] = {"median": round(statistics.median(ratios), 4), "min": round(min(ratios), 4),
                                           "max": round(max(ratios), 4)}
    res["gated"] = gated
    res["gate_met"] = res["vread_time_over_composed"]["median"] < 1.0 if gated else None
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--block", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="a,au,b,bu,c,cu,d,e")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vread", "vread_rate.jsonl"))
    ap.add_argument("--limit", type=int, default=420, help="seconds a case may take")
    ap.add_argument("--case", choices=sorted(CASES), help="run this one case in this process (the driver's child)")
    args = ap.parse_args()
    if args.case:
        return run_case(args, args.case)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    missed = []
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
        if json.loads(line)["gate_met"] is False:
            missed.append(case)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    if missed:
        sys.exit(f"the gate (vread / composed < 1, median) was missed in case(s) {','.join(missed)}")


if __name__ == "__main__":
    main()
