#!/usr/bin/env python3
"""Piece-checksum rate against the block checksums and the scrub, in one process: RS(10,4), 1 MiB blocks, 4096
stripes resident in HBM.

Times, by HIP events after a warm-up, rounds whose legs alternate, so that box-to-box and minute-to-minute drift hits
them alike:
  scrub     ecg_scrub.encode_batch over the stripes: the read-only pass over these bytes the project already has;
  sum       ecg_sum.blocks_batch over the same stripes: the same 14 * B bytes per stripe, one sum per block;
  p512, p4k, p64k, p1m
            ecg_psum.pieces_batch at piece sizes 512 B, 4 KiB, 64 KiB and 1 MiB;
  pverify4k ecg_psum.verify_batch at 4 KiB against the sums of p4k;
  control   the scrub a second time.
The yardsticks are the same run's scrub and block sums.  Prints ONE JSON line and appends it to --out: per leg the
bytes read, median / min / max ms and the fraction of 8 TB/s; per round the ratios leg / sum and leg / scrub (time over
time, same bytes) with their median, min and max, the control's among them.  Asserts that the stripes are clean, that
every verify names no block, that the piece sums are reproducible, that every piece size folds to the block sums
(ecg_psum.fold over a sample), and that ecg_psum.counters() moved by S * B * 14 bytes per call.
Needs the GPU: there is no CPU path.  One case per process: run it again for another span.

    python tools/psum_rate.py [--stripes 4096] [--block 1048576] [--rounds 10] [--warmup 2] [--span 0] [--note TEXT]
                              [--out profiles/psum/psum_rate.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "erasure-codes-prototype_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK = 8.0e12  # MI355X HBM3E peak, bytes per second
PIECES = (("p512", 512), ("p4k", 4 << 10), ("p64k", 64 << 10), ("p1m", 1 << 20))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--block", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--span", type=int, default=0, help="ecg_psum.set_span_bytes (0 = auto)")
    ap.add_argument("--note", default="", help="recorded in the line as it is (which build, which case)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "psum", "psum_rate.jsonl"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import ecg
    import ecg_psum
    import ecg_scrub
    import ecg_sum

    if not torch.cuda.is_available():
        sys.exit("psum_rate.py needs an MI355X (torch.cuda.is_available() is False)")
    torch.cuda.set_device(0)
    k, m, S, B = 10, 4, args.stripes, args.block
    n = k + m
    M = ecg.reed_sol_vandermonde_coding_matrix(k, m)
    stripes = torch.empty((S, n, B), dtype=torch.uint8, device="cuda")
    counts = torch.empty((S, m), dtype=torch.int32, device="cuda")
    sums = torch.empty((S, n), dtype=torch.int32, device="cuda")
    ecg.fill_random(stripes, 0x5C2B)
    ecg.encode_batch(k, m, M, stripes[:, :k], stripes[:, k:])
    ecg_psum.set_span_bytes(args.span)
    ids = list(range(n))
    out_of = {name: torch.empty((S, n, ecg_psum.pieces(B, P)), dtype=torch.int32, device="cuda") for name, P in PIECES}
    recorded = {}
    for name, P in PIECES:
        ecg_psum.pieces_batch(ids, stripes, P, out=out_of[name])
        recorded[name] = out_of[name].clone()
    checked = torch.empty_like(recorded["p4k"])
    ecg_sum.blocks_batch(ids, stripes, out=sums)
    torch.cuda.synchronize()
    verdict = []

    def scrub():
        ecg_scrub.encode_batch(k, m, M, stripes, out=counts)

    def block_sums():
        ecg_sum.blocks_batch(ids, stripes, out=sums)

    def pieces_of(name, P):
        return lambda: ecg_psum.pieces_batch(ids, stripes, P, out=out_of[name])

    def verify():
        verdict.append(ecg_psum.verify_batch(ids, stripes, 4 << 10, recorded["p4k"], out=checked)[1:])

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    legs = (("scrub", scrub), ("sum", block_sums)) + tuple((name, pieces_of(name, P)) for name, P in PIECES) + \
           (("pverify4k", verify), ("control", scrub))
    ms = {name: [] for name, _ in legs}
    for _ in range(args.warmup):
        for _, fn in legs:
            fn()
    torch.cuda.synchronize()
    verdict.clear()
    c0 = ecg_psum.counters()
    for _ in range(args.rounds):
        for name, fn in legs:
            ms[name].append(timed(fn))
    c1 = ecg_psum.counters()
    launches = {}
    for name, P in PIECES:                                   # the geometry of each piece size, outside the timing
        ecg_psum.pieces_batch(ids, stripes, P, out=out_of[name])
        launches[name] = ecg_psum.last_launch()
    torch.cuda.synchronize()
    assert c1["bytes"] - c0["bytes"] == (len(PIECES) + 1) * args.rounds * S * B * n, (c0, c1)
    assert not counts.any().item(), "clean stripes reported a nonzero count"
    for name, _ in PIECES:
        assert torch.equal(out_of[name], recorded[name]), "the piece sums are not reproducible"
    assert torch.equal(checked, recorded["p4k"])
    for targets, bad in verdict:
        assert (targets == -1).all().item() and not bad.any().item()
    block = sums.cpu().numpy().view(np.uint32)
    for name, P in PIECES:                                   # every piece size folds to the block sums
        for s in range(0, S, max(1, S // 8)):
            got = recorded[name][s].cpu().numpy().view(np.uint32)
            for j in (0, n - 1):
                assert ecg_psum.fold(got[j], P, B) == int(block[s, j]), (name, s, j)

    moved = S * B * n
    out = {"tool": "psum_rate", "code": "RS(10,4)", "stripes": S, "block_bytes": B, "rounds": args.rounds,
           "warmup": args.warmup, "peak_bytes_per_s": PEAK, "device": torch.cuda.get_device_name(0),
           "span_asked": args.span, "note": args.note, "last_launch": launches}
    for name, v in ms.items():
        med = statistics.median(v)
        out[name] = {"bytes": moved, "ms": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                     "frac_of_8TBps": round(moved / (med * 1e-3) / PEAK, 4)}
        for base in ("sum", "scrub"):
            if name != base:
                r = [a / b for a, b in zip(v, ms[base])]
                out[name]["time_over_%s_per_round" % base] = {"median": round(statistics.median(r), 4),
                                                               "min": round(min(r), 4), "max": round(max(r), 4)}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
