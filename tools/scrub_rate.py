#!/usr/bin/env python3
"""Scrub rate against the encode, in one process: RS(10,4), 1 MiB blocks, 4096 stripes resident in HBM.

Times, by HIP events after a warm-up, rounds of
  (a) ecg.encode_batch as shipped (parity written into the stripes);
  (b) ecg_scrub.encode_batch on clean stripes;
  (d) today's alternative: encode into a scratch parity area + torch.equal against the stored parity;
then, with one data block of EVERY stripe corrupted in every byte (every workgroup issues its atomics: their worst
case),
  (c) ecg_scrub.encode_batch on the corrupt stripes.
(a), (b) and (d) alternate within a round, so box-to-box and minute-to-minute drift hits them alike.  Prints ONE JSON
line: bytes moved, median / min / max ms and the fraction of 8 TB/s for each, and the scrub's bytes per second over
the same run's encode.  Asserts the counts (all zero when clean, B per row and stripe when corrupt) and that
ecg_scrub.counters() moved by S * B * 14 bytes per scrub.  Needs the GPU: there is no CPU path.

    python tools/scrub_rate.py [--stripes 4096] [--block 1048576] [--rounds 20] [--warmup 3]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--block", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch

    import ecg
    import ecg_scrub

    if not torch.cuda.is_available():
        sys.exit("scrub_rate.py needs an MI355X (torch.cuda.is_available() is False)")
    torch.cuda.set_device(0)
    k, m, S, B = 10, 4, args.stripes, args.block
    n = k + m
    M = ecg.reed_sol_vandermonde_coding_matrix(k, m)
    stripes = torch.empty((S, n, B), dtype=torch.uint8, device="cuda")
    scratch = torch.empty((S, m, B), dtype=torch.uint8, device="cuda")
    counts = torch.empty((S, m), dtype=torch.int32, device="cuda")
    ecg.fill_random(stripes, 0x5C2B)
    data, parity = stripes[:, :k], stripes[:, k:]
    ecg.encode_batch(k, m, M, data, parity)
    torch.cuda.synchronize()

    def encode():
        ecg.encode_batch(k, m, M, data, parity)

    def scrub():
        ecg_scrub.encode_batch(k, m, M, stripes, out=counts)

    equal = []

    def encode_compare():
        ecg.encode_batch(k, m, M, data, scratch)
        equal.append(torch.equal(scratch, parity))

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    ms = {"encode": [], "scrub_clean": [], "scrub_corrupt": [], "encode_plus_equal": []}
    for _ in range(args.warmup):
        encode(), scrub(), encode_compare()
    torch.cuda.synchronize()
    c0 = ecg_scrub.counters()
    for _ in range(args.rounds):
        ms["encode"].append(timed(encode))
        ms["scrub_clean"].append(timed(scrub))
        ms["encode_plus_equal"].append(timed(encode_compare))
    c1 = ecg_scrub.counters()
    assert c1["bytes"] - c0["bytes"] == args.rounds * S * B * n, (c0, c1)
    assert c1["launches"] - c0["launches"] == args.rounds
    assert not counts.any().item(), "clean stripes reported a nonzero count"
    assert all(equal)

    stripes[:, 3] ^= 0x5A  # every byte of data block 3 of every stripe
    for _ in range(args.warmup):
        scrub()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        ms["scrub_corrupt"].append(timed(scrub))
    assert (counts == B).all().item(), "a nonzero coefficient times a nonzero byte is nonzero: B per row and stripe"
    stripes[:, 3] ^= 0x5A
    scrub()
    assert not counts.any().item()

    moved = {"encode": S * B * n, "scrub_clean": S * B * n, "scrub_corrupt": S * B * n,
             "encode_plus_equal": S * B * (n + 2 * m)}  # encode reads k, writes m; the compare reads 2 m
    out = {"tool": "scrub_rate", "code": "RS(10,4)", "stripes": S, "block_bytes": B, "rounds": args.rounds,
           "warmup": args.warmup, "peak_bytes_per_s": PEAK, "device": torch.cuda.get_device_name(0)}
    for name, v in ms.items():
        med = statistics.median(v)
        out[name] = {"bytes": moved[name], "ms": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                     "frac_of_8TBps": round(moved[name] / (med * 1e-3) / PEAK, 4)}
    for name in ("scrub_clean", "scrub_corrupt"):
        out[name]["bytes_per_s_over_encode"] = round(out["encode"]["ms"] / out[name]["ms"], 4)  # same bytes moved
    out["encode_plus_equal"]["time_over_scrub_clean"] = round(
        out["encode_plus_equal"]["ms"] / out["scrub_clean"]["ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
