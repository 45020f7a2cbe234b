#!/usr/bin/env python3
"""The tail of a sketch call -- sort, unique, read-back -- on three inputs, with the sort that served them (sort_counters(), where
the library has them): the C2 batch of bench.py, a 4.6 MB buffer (one bacterial genome per call: microseconds per
DeviceSketcher.sketch call, five batches of 200), and kept hashes that do not spread (a 150-base period repeated to 2 x 10^9
bytes at scaled = 100; of this period's k-mers exactly one hash is kept, 1.3 x 10^7 times: the uniform sort tries, gives up on the
device, and the general sort runs behind it).
python tools/bench_sort_path.py [c2] [small] [period]      (default: all three); prints one JSON line"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def counters(smd):
    return smd.sort_counters() if hasattr(smd, "sort_counters") else None


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def main():
    import torch
    from sourmash_amd import device as smd
    what = sys.argv[1:] or ["c2", "small", "period"]
    out = {}
    if "c2" in what:
        seq = smd.synth_dna(10_000_001_000, seed=42, record_len=10_000_000)
        sk = smd.DeviceSketcher(31, 1000)
        c0 = counters(smd)
        dt, h = timed(torch, lambda: sk.sketch(seq), 5)
        out["c2_ms_per_call"] = round(dt * 1e3, 3)
        out["c2_hashes"] = int(h.numel())
        out["c2_sort_counters"] = None if c0 is None else {k: v - c0[k] for k, v in counters(smd).items()}
        del seq, sk
    if "small" in what:
        seq = smd.synth_dna(4_600_000, seed=42, record_len=10_000_000)
        sk = smd.DeviceSketcher(31, 1000)
        c0 = counters(smd)
        batches = []
        for _ in range(5):
            dt, h = timed(torch, lambda: sk.sketch(seq), 200)
            batches.append(round(dt * 1e6, 2))
        out["small_4p6MB_us_per_call"] = batches
        out["small_hashes"] = int(h.numel())
        out["small_sort_counters"] = None if c0 is None else {k: v - c0[k] for k, v in counters(smd).items()}
    if "period" in what:
        n = 2_000_000_000
        import numpy as np
        period = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(6).integers(0, 4, size=150)]
        seq = torch.from_numpy(period.copy()).cuda().repeat(n // 150 + 1)[:n].contiguous()
        sk = smd.DeviceSketcher(31, 100)
        c0 = counters(smd)
        dt, h = timed(torch, lambda: sk.sketch(seq), 3)
        out["period150_ms_per_call"] = round(dt * 1e3, 3)
        out["period150_Gbyte_per_s"] = round(n / dt / 1e9, 2)
        out["period150_hashes"] = int(h.numel())
        out["period150_sort_counters"] = None if c0 is None else {k: v - c0[k] for k, v in counters(smd).items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
