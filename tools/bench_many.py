#!/usr/bin/env python3
"""Many queries against the C5 collection: SketchSet.overlaps_many (one pass over the collection for all queries) against the loop of
SketchSet.overlaps (one pass per query) over the same queries in the same process.

    python tools/bench_many.py [--rows 100000] [--row-size 5000] [--m 1 64 1000] [--reps 7] [--min-common 50]
                               [--time-limit 900] [--out profiles/many_bench.json]

Database: the C5 set of synth.synth_gather_device (100,000 rows of about 5,000 hashes, 4 GB).  Queries: m rows of the same family
(half of a row's hashes come from the shared million-hash pool, so an unrelated pair shares a handful), every fourth one a copy of
a database row, so that a few pairs clear the threshold.  Both sides report the pairs sharing at least --min-common hashes; the
results are compared before anything is timed.  Per m: the whole overlaps_many call (host clock, arrays fetched), its index build,
its passes and its final sort (device events), and the loop with its thresholding; medians of --reps runs, every run kept.
Needs a GPU; stops itself after --time-limit seconds."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--row-size", type=int, default=5000)
    ap.add_argument("--m", type=int, nargs="+", default=[1, 64, 1000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-common", type=int, default=50)
    ap.add_argument("--time-limit", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "many_bench.json"))
    args = ap.parse_args()

    def out_of_time(*_):
        print(f"bench_many: the time limit of {args.time_limit} s ran out", file=sys.stderr, flush=True)
        os._exit(3)
    signal.signal(signal.SIGALRM, out_of_time)
    signal.alarm(args.time_limit)

    import numpy as np
    import torch
    import sourmash_amd as sm
    from sourmash_amd.synth import synth_gather_device
    assert sm.gpu_available(), "no HIP device visible"
    dev = torch.device("cuda:0")
    n = args.rows
    _, hashes, offsets = synth_gather_device(1_000_000, n, args.row_size, dev)
    db = sm.SketchSet.from_csr(hashes, offsets, ksize=31, scaled=1000)
    total = int(offsets[-1])
    del hashes, offsets
    result = {"device": torch.cuda.get_device_name(0), "rows": n, "total_hashes": total, "min_common": args.min_common, "reps": args.reps,
              "what": "ms; many_call = SketchSet.overlaps_many end to end (host clock), build / kernel / sort = its device phases (events), "
                      "loop = SketchSet.overlaps per query + thresholding; ratio = loop median / many_call median (above 1: the one pass wins)",
              "results": []}
    for m in args.m:
        # m rows of the family behind the database's own, every fourth one replaced by a copy of a database row
        _, qh, qoff = synth_gather_device(1_000_000, n + m, args.row_size, dev, row_lo=n, row_hi=n + m)
        extra = sm.SketchSet.from_csr(qh, qoff, ksize=31, scaled=1000)
        mhs = [extra.minhash(i) if i % 4 else db.minhash((97 * i + 13) % n) for i in range(m)]
        qs = sm.SketchSet(mhs)
        q_total = qs.total_hashes

        def many():
            t0 = time.perf_counter()
            hits = db._many_hits(qs, args.min_common)
            arrays = (hits.queries, hits.rows, hits.common)
            return (time.perf_counter() - t0) * 1e3, hits.stats, arrays

        def loop():
            t0 = time.perf_counter()
            found = []
            for q, mh in enumerate(mhs):
                c = db.overlaps(mh)
                rows = np.flatnonzero(c >= args.min_common)
                found.append((np.full(len(rows), q), rows, c[rows]))
            ms = (time.perf_counter() - t0) * 1e3
            return ms, tuple(np.concatenate([f[i] for f in found]) for i in range(3))

        _, stats, got = many()                                          # warm-up, and the comparison
        _, want = loop()
        agree = all(np.array_equal(a.astype(np.int64), b.astype(np.int64)) for a, b in zip(got, want))
        assert agree, f"m = {m}: the one pass and the loop disagree"
        runs = {"many_call": [], "build": [], "kernel": [], "sort": [], "loop": []}
        for _ in range(args.reps):
            ms, stats, _ = many()
            runs["many_call"].append(ms)
            for k in ("build", "kernel", "sort"):
                runs[k].append(stats[k + "_ms"])
            runs["loop"].append(loop()[0])
        med = {k: statistics.median(v) for k, v in runs.items()}
        row = {"m": m, "query_hashes": int(q_total), "hits": int(len(got[0])), "agree": agree, "passes": int(stats["passes"]), "reruns": int(stats["reruns"]),
               "median_ms": {k: round(v, 3) for k, v in med.items()}, "runs_ms": {k: [round(x, 3) for x in v] for k, v in runs.items()},
               "ratio_loop_over_many": round(med["loop"] / med["many_call"], 3), "loop_ms_per_query": round(med["loop"] / m, 3)}
        result["results"].append(row)
        print(json.dumps({k: row[k] for k in ("m", "hits", "median_ms", "ratio_loop_over_many", "loop_ms_per_query")}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
