#!/usr/bin/env python3
"""Block-checksum rate against the scrub, in one process: RS(10,4), 1 MiB blocks, 4096 stripes resident in HBM.

Times, by HIP events after a warm-up, rounds whose legs alternate, so that box-to-box and minute-to-minute drift hits
them alike:
  (a) ecg_scrub.encode_batch over the stripes: the read-only pass over these bytes the project already has;
  (b) ecg_sum.blocks_batch over the same stripes: the same 14 * B bytes per stripe;
  (c) ecg_sum.verify_batch against the sums of (b);
  (d) a control: the scrub a second time.
The yardstick is the same run's scrub.  Prints ONE JSON line and appends it to --out: per leg the bytes read, median /
min / max ms and the fraction of 8 TB/s; per round the ratios sum / scrub and control / scrub (time over time, same
bytes), with their median, min and max; and one CPU figure, ecg_sum.crc32c over a sample of the blocks from 16
threads, scaled to the whole store and labelled as such.  Asserts that the stripes are clean, that every verify names
no block, that a sample of the sums equals the CPU's, and that ecg_sum.counters() moved by S * B * 14 bytes per sum.
Needs the GPU: there is no CPU path.  One case per process: run it again for another segment size.

    python tools/sum_rate.py [--stripes 4096] [--block 1048576] [--rounds 20] [--warmup 3] [--segment 0] [--scheme -1]
                             [--note TEXT] [--out profiles/sum/sum_rate.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "erasure-codes-prototype_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK = 8.0e12  # MI355X HBM3E peak, bytes per second
CPU_THREADS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--block", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--segment", type=int, default=0, help="ecg_sum.set_segment_bytes (0 = auto)")
    ap.add_argument("--scheme", type=int, default=-1, help="ecg_sum.set_table_scheme (-1 = auto)")
    ap.add_argument("--note", default="", help="recorded in the line as it is (which build, which case)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sum", "sum_rate.jsonl"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import ecg
    import ecg_scrub
    import ecg_sum

    if not torch.cuda.is_available():
        sys.exit("sum_rate.py needs an MI355X (torch.cuda.is_available() is False)")
    torch.cuda.set_device(0)
    k, m, S, B = 10, 4, args.stripes, args.block
    n = k + m
    M = ecg.reed_sol_vandermonde_coding_matrix(k, m)
    stripes = torch.empty((S, n, B), dtype=torch.uint8, device="cuda")
    counts = torch.empty((S, m), dtype=torch.int32, device="cuda")
    sums = torch.empty((S, n), dtype=torch.int32, device="cuda")
    checked = torch.empty((S, n), dtype=torch.int32, device="cuda")
    ecg.fill_random(stripes, 0x5C2B)
    ecg.encode_batch(k, m, M, stripes[:, :k], stripes[:, k:])
    ecg_sum.set_segment_bytes(args.segment)
    ecg_sum.set_table_scheme(args.scheme)
    ids = list(range(n))
    ecg_sum.blocks_batch(ids, stripes, out=sums)
    torch.cuda.synchronize()
    recorded = sums.clone()
    verdict = []

    def scrub():
        ecg_scrub.encode_batch(k, m, M, stripes, out=counts)

    def block_sums():
        ecg_sum.blocks_batch(ids, stripes, out=sums)

    def verify():
        verdict.append(ecg_sum.verify_batch(ids, stripes, recorded, out=checked)[1:])

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    legs = (("scrub", scrub), ("sum", block_sums), ("verify", verify), ("control", scrub))
    ms = {name: [] for name, _ in legs}
    for _ in range(args.warmup):
        for _, fn in legs:
            fn()
    torch.cuda.synchronize()
    verdict.clear()
    c0 = ecg_sum.counters()
    for _ in range(args.rounds):
        for name, fn in legs:
            ms[name].append(timed(fn))
    c1 = ecg_sum.counters()
    last = ecg_sum.last_launch()
    assert c1["bytes"] - c0["bytes"] == 2 * args.rounds * S * B * n, (c0, c1)
    assert not counts.any().item(), "clean stripes reported a nonzero count"
    assert torch.equal(sums, recorded) and torch.equal(checked, recorded), "the sums are not reproducible"
    for targets, bad in verdict:
        assert (targets == -1).all().item() and not bad.any().item()

    # the CPU figure, and a check of the GPU's sums on the way: a sample of blocks through ecg_sum.crc32c
    sample = [(s, j) for s in range(0, S, max(1, S // 16)) for j in (0, n - 1)][:2 * CPU_THREADS]
    host = [stripes[s, j].cpu().numpy() for s, j in sample]
    ecg_sum.crc32c(host[0])
    t0 = time.perf_counter()
    with ThreadPoolExecutor(CPU_THREADS) as pool:
        cpu = list(pool.map(ecg_sum.crc32c, host))
    cpu_s = time.perf_counter() - t0
    got = recorded.cpu().numpy().view(np.uint32)
    assert [int(got[s, j]) for s, j in sample] == cpu, "GPU and CPU sums differ"

    moved = S * B * n
    out = {"tool": "sum_rate", "code": "RS(10,4)", "stripes": S, "block_bytes": B, "rounds": args.rounds,
           "warmup": args.warmup, "peak_bytes_per_s": PEAK, "device": torch.cuda.get_device_name(0),
           "segment_asked": args.segment, "scheme_asked": args.scheme, "note": args.note, "last_launch": last}
    for name, v in ms.items():
        med = statistics.median(v)
        out[name] = {"bytes": moved, "ms": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                     "frac_of_8TBps": round(moved / (med * 1e-3) / PEAK, 4)}
    for name in ("sum", "verify", "control"):
        r = [a / b for a, b in zip(ms[name], ms["scrub"])]
        out[name]["time_over_scrub_per_round"] = {"median": round(statistics.median(r), 4), "min": round(min(r), 4),
                                                  "max": round(max(r), 4)}
    cpu_rate = len(host) * B / cpu_s
    out["cpu_crc32c_16_threads"] = {
        "note": "ecg_sum.crc32c over a sample of blocks from 16 host threads, scaled to the store; not a GPU figure",
        "sample_blocks": len(host), "bytes_per_s": round(cpu_rate),
        "ms_scaled_to_the_store": round(moved / cpu_rate * 1e3, 1)}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
