#!/usr/bin/env python3
"""Gather of many queries against the C5 collection: SketchSet.gather_many (one candidate pass over the collection, then the
min-set-cover loops of all queries side by side) against the loop of SketchSet.gather (one index build and one resident loop per
query) over the same queries in the same process.

    python tools/bench_gather_many.py [--rows 100000] [--row-size 5000] [--m 1 64 1000] [--reps 7] [--threshold-bp 50000]
                                      [--time-limit 900] [--out profiles/gather_many_bench.json]

Database and queries: those of tools/bench_many.py -- the C5 set of synth.synth_gather_device (100,000 rows of about 5,000 hashes,
4 GB), and m rows of the same family (half of a row's hashes come from the shared million-hash pool, so an unrelated pair shares a
handful), every fourth one a copy of a database row.  The results are compared before anything is timed.  Per m: the whole
gather_many call (host clock, picks fetched), its candidate pass, fill, sort and rounds kernel (device events), its one-query way out,
and the loop; medians of --reps runs, every run kept.  Needs a GPU; stops itself after --time-limit seconds."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ("candidates", "fill", "sort", "rounds", "way_out")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--row-size", type=int, default=5000)
    ap.add_argument("--m", type=int, nargs="+", default=[1, 64, 1000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threshold-bp", type=int, default=50_000)
    ap.add_argument("--time-limit", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather_many_bench.json"))
    args = ap.parse_args()

    def out_of_time(*_):
        print(f"bench_gather_many: the time limit of {args.time_limit} s ran out", file=sys.stderr, flush=True)
        os._exit(3)
    signal.signal(signal.SIGALRM, out_of_time)
    signal.alarm(args.time_limit)

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
    result = {"device": torch.cuda.get_device_name(0), "rows": n, "total_hashes": total, "threshold_bp": args.threshold_bp, "reps": args.reps,
              "what": "ms; many_call = SketchSet.gather_many end to end (host clock), candidates / fill / sort / rounds = its device phases "
                      "(events), way_out = its one-query path (host clock), loop = SketchSet.gather per query; ratio = loop median / "
                      "many_call median (above 1: the one call wins); separated = the recorded ranges of the two do not overlap",
              "results": []}
    for m in args.m:
        # m rows of the family behind the database's own, every fourth one replaced by a copy of a database row
        _, qh, qoff = synth_gather_device(1_000_000, n + m, args.row_size, dev, row_lo=n, row_hi=n + m)
        extra = sm.SketchSet.from_csr(qh, qoff, ksize=31, scaled=1000)
        mhs = [extra.minhash(i) if i % 4 else db.minhash((97 * i + 13) % n) for i in range(m)]
        qs = sm.SketchSet(mhs)

        def many():
            t0 = time.perf_counter()
            res = db._many_gather(qs, args.threshold_bp)
            picks = res.per_query()
            return (time.perf_counter() - t0) * 1e3, res.stats, picks

        def loop():
            t0 = time.perf_counter()
            picks = [db.gather(mh, args.threshold_bp) for mh in mhs]
            return (time.perf_counter() - t0) * 1e3, picks

        _, stats, got = many()                                          # warm-up, and the comparison
        _, want = loop()
        agree = got == want
        assert agree, f"m = {m}: the one call and the loop disagree"
        runs = {k: [] for k in ("many_call",) + PHASES + ("loop",)}
        for _ in range(args.reps):
            ms, stats, _ = many()
            runs["many_call"].append(ms)
            for k in PHASES:
                runs[k].append(stats[k + "_ms"])
            runs["loop"].append(loop()[0])
        med = {k: statistics.median(v) for k, v in runs.items()}
        row = {"m": m, "query_hashes": int(qs.total_hashes), "picks": sum(len(p) for p in got), "queries_with_picks": sum(1 for p in got if p),
               "agree": agree, "batches": int(stats["batches"]), "way_out_queries": int(stats["way_out_queries"]),
               "median_ms": {k: round(v, 3) for k, v in med.items()}, "runs_ms": {k: [round(x, 3) for x in v] for k, v in runs.items()},
               "ratio_loop_over_many": round(med["loop"] / med["many_call"], 3), "loop_ms_per_query": round(med["loop"] / m, 3),
               "separated": bool(max(runs["many_call"]) < min(runs["loop"]) or max(runs["loop"]) < min(runs["many_call"]))}
        result["results"].append(row)
        print(json.dumps({k: row[k] for k in ("m", "picks", "median_ms", "ratio_loop_over_many", "loop_ms_per_query", "separated")}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
