#!/usr/bin/env python3
"""The result rows of gather for many abundance queries against the C5 collection: SketchSet.gather_stats_many + GatherStats.rows (the
many-queries gather, one more pass over the resident sets, rows from integers) against the loop of GatherDatabases + gatherresultdict
(MinHash objects and a dictionary walk per round) over the same queries in the same process.

    python tools/bench_gather_rows.py [--rows 100000] [--row-size 5000] [--m 1 64 1000] [--reps 7] [--threshold-bp 50000]
                                      [--loop-queries 32] [--big-rounds 3] [--time-limit 900] [--out profiles/gather_rows_bench.json]

Database and queries: those of tools/bench_gather_many.py (the C5 set, m rows of the same family, every fourth one a copy of a database
row), each query hash with an abundance of 1 .. 50.  Then the 10^6-hash C5 query alone through SketchSet.gather_stats.  The loop's
CounterGather is built from the query's candidates (SketchSet.prefetch, the rows as signatures) outside the clock: what is timed is
the iteration of GatherDatabases and gatherresultdict, the code the native rows replace.  The loop runs on the first --loop-queries
queries and is scaled to m (the JSON says on how many it ran); for the C5 query its counter holds the picked rows only (the picks are
the same: every round's winner is among them) and only its first --big-rounds rounds are timed.  A round walks the remaining query,
which shrinks as the picks leave it, so those rounds scaled to all rounds are an upper estimate of the loop, recorded as one; no
ratio is formed from it.  The rows are
compared, every column by ==, before anything is timed.  Medians of --reps runs, every run kept.  Needs a GPU."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("gather", "owner", "tally", "sort", "call")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--row-size", type=int, default=5000)
    ap.add_argument("--m", type=int, nargs="+", default=[1, 64, 1000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threshold-bp", type=int, default=50_000)
    ap.add_argument("--loop-queries", type=int, default=32)
    ap.add_argument("--big-rounds", type=int, default=3)
    ap.add_argument("--time-limit", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather_rows_bench.json"))
    args = ap.parse_args()

    def out_of_time(*_):
        print(f"bench_gather_rows: the time limit of {args.time_limit} s ran out", file=sys.stderr, flush=True)
        os._exit(3)
    signal.signal(signal.SIGALRM, out_of_time)
    signal.alarm(args.time_limit)

    import numpy as np
    import torch
    import sourmash_amd as sm
    from sourmash_amd.index import CounterGather
    from sourmash_amd.search import GatherDatabases
    from sourmash_amd.synth import synth_gather_device
    assert sm.gpu_available(), "no HIP device visible"
    dev = torch.device("cuda:0")
    n = args.rows
    big_query, hashes, offsets = synth_gather_device(1_000_000, n, args.row_size, dev)
    db = sm.SketchSet.from_csr(hashes, offsets, ksize=31, scaled=1000, names=[f"row{i}" for i in range(n)], filenames=["c5.zip"] * n)
    total = int(offsets[-1])
    del hashes, offsets
    rng = np.random.default_rng(7)

    def with_abundance(mh):
        out = sm.MinHash(0, mh.ksize, scaled=mh.scaled, track_abundance=True)
        hs = sorted(mh.hashes)
        ab = rng.integers(1, 51, size=len(hs), dtype=np.uint64)
        out.set_abundances(dict(zip(hs, ab.tolist())))
        return out, ab

    def counter_for(sig, rows):
        flat = sig.to_mutable()
        flat.minhash = flat.minhash.flatten()
        counter = CounterGather(flat)
        counter.add_many([db.signature(r) for r in rows], locations=["c5.zip"] * len(rows))
        return counter

    def loop_rows(sig, counter, rounds=None):
        "-> (ms of the iteration and the dicts, the dicts)"
        t0 = time.perf_counter()
        out = []
        for r in GatherDatabases(sig, [counter], threshold_bp=args.threshold_bp):
            out.append(r.gatherresultdict)
            if rounds is not None and len(out) >= rounds:
                break
        return (time.perf_counter() - t0) * 1e3, out

    result = {"device": torch.cuda.get_device_name(0), "rows": n, "total_hashes": total, "threshold_bp": args.threshold_bp, "reps": args.reps,
              "what": "ms; native_call = SketchSet.gather_stats_many end to end (host clock), gather / owner / tally / sort = its steps (gather: host "
                      "clock of the many-queries gather inside it; the three others device events), rows = GatherStats.rows (host), gather_many = "
                      "SketchSet.gather_many alone (host clock) and candidates = its candidate pass (device events); loop = the iteration of "
                      "GatherDatabases + gatherresultdict over loop_queries queries scaled to m (counters built outside the clock); "
                      "pass_share = (owner + tally + sort) / native_call; ratio = loop / (native_call + rows)",
              "results": []}
    for m in args.m:
        _, qh, qoff = synth_gather_device(1_000_000, n + m, args.row_size, dev, row_lo=n, row_hi=n + m)
        extra = sm.SketchSet.from_csr(qh, qoff, ksize=31, scaled=1000)
        pairs = [with_abundance(extra.minhash(i) if i % 4 else db.minhash((97 * i + 13) % n)) for i in range(m)]
        mhs, abunds = [p[0] for p in pairs], [p[1] for p in pairs]
        qs = sm.SketchSet([mh.flatten() for mh in mhs])
        qs.set_names([f"query{i}" for i in range(m)], ["queries.sig"] * m)
        sigs = [sm.SourmashSignature(mh, name=f"query{i}", filename="queries.sig") for i, mh in enumerate(mhs)]

        def native():
            t0 = time.perf_counter()
            stats = db.gather_stats_many(qs, args.threshold_bp, abunds=abunds)
            t1 = time.perf_counter()
            rows = stats.rows()
            return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, stats, rows

        _, _, stats, got = native()                                     # warm-up, and the comparison
        k = min(m, args.loop_queries)
        counters = lambda: [counter_for(sigs[q], [r for r, _ in db.prefetch(mhs[q].flatten(), args.threshold_bp)]) for q in range(k)]   # noqa: E731
        want = [loop_rows(sigs[q], c)[1] for q, c in enumerate(counters())]
        agree = got[:k] == want
        assert agree, f"m = {m}: the native rows and the loop's disagree"
        runs = {key: [] for key in ("native_call", "rows", "gather_many", "candidates", "loop") + STEPS[:4]}
        for _ in range(args.reps):
            call_ms, rows_ms, stats, _ = native()
            runs["native_call"].append(call_ms)
            runs["rows"].append(rows_ms)
            for key in STEPS[:4]:
                runs[key].append(stats.stats[key + "_ms"])
            t0 = time.perf_counter()
            res = db._many_gather(qs, args.threshold_bp)
            res.per_query()
            runs["gather_many"].append((time.perf_counter() - t0) * 1e3)
            runs["candidates"].append(res.stats["candidates_ms"])
            cs = counters()
            runs["loop"].append(sum(loop_rows(sigs[q], c)[0] for q, c in enumerate(cs)) * m / k)
        med = {key: statistics.median(v) for key, v in runs.items()}
        device_pass = med["owner"] + med["tally"] + med["sort"]
        row = {"m": m, "query_hashes": int(qs.total_hashes), "picks": int(stats.offsets[-1]), "loop_queries": k, "agree": agree,
               "median_ms": {key: round(v, 3) for key, v in med.items()}, "runs_ms": {key: [round(x, 3) for x in v] for key, v in runs.items()},
               "pass_ms": round(device_pass, 3), "pass_share_of_call": round(device_pass / med["native_call"], 4),
               "pass_below_candidate_pass": bool(device_pass < med["candidates"]),
               "ratio_loop_over_native": round(med["loop"] / (med["native_call"] + med["rows"]), 2)}
        result["results"].append(row)
        print(json.dumps({key: row[key] for key in ("m", "picks", "median_ms", "pass_ms", "pass_below_candidate_pass", "ratio_loop_over_native")}), flush=True)

    # ---- the C5 query alone: 10^6 hashes, about 1,500 rounds
    big = sm.MinHash(0, 31, scaled=1000, track_abundance=True)
    hs = big_query.cpu().numpy().view(np.uint64)
    big_ab = rng.integers(1, 51, size=len(hs), dtype=np.uint64)
    big.set_abundances(dict(zip(hs.tolist(), big_ab.tolist())))
    sig = sm.SourmashSignature(big, name="c5 query", filename="c5.sig")

    def native_big():
        t0 = time.perf_counter()
        stats = db.gather_stats(big, args.threshold_bp)
        t1 = time.perf_counter()
        stats.query_info = [dict(query_name=sig.name, query_filename=sig.filename, query_md5=sig.md5sum()[:8])]
        rows = stats.rows()
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, stats, rows

    _, _, stats, got = native_big()
    picked = stats.pick_rows.tolist()
    rounds = min(args.big_rounds, len(picked))
    _, want = loop_rows(sig, counter_for(sig, sorted(picked)), rounds)
    agree = got[0][:rounds] == want
    assert agree, "the C5 query: the native rows and the loop's disagree"
    # The loop's baseline is its FIRST rounds only.  A round walks the remaining query, which is largest in these rounds and shrinks
    # as the picks leave it, so first rounds x (picks / rounds) is an UPPER estimate of the whole loop, not a measurement of it: it
    # is recorded as such, beside the time of the rounds that were run, and no ratio is formed from it.
    runs = {key: [] for key in ("native_call", "rows", "loop_first_rounds") + STEPS[:4]}
    for rep in range(args.reps):
        call_ms, rows_ms, stats, _ = native_big()
        runs["native_call"].append(call_ms)
        runs["rows"].append(rows_ms)
        for key in STEPS[:4]:
            runs[key].append(stats.stats[key + "_ms"])
        if rep < 3:                                                     # (a round of the loop walks the million-hash dictionary)
            runs["loop_first_rounds"].append(loop_rows(sig, counter_for(sig, sorted(picked)), rounds)[0])
    med = {key: statistics.median(v) for key, v in runs.items()}
    row = {"query": "c5", "query_hashes": len(hs), "picks": len(picked), "loop_rounds_timed": rounds, "loop_runs": len(runs["loop_first_rounds"]), "agree": agree,
           "median_ms": {key: round(v, 3) for key, v in med.items()}, "runs_ms": {key: [round(x, 3) for x in v] for key, v in runs.items()},
           "pass_ms": round(med["owner"] + med["tally"] + med["sort"], 3),
           "loop_all_rounds_upper_estimate_ms": round(med["loop_first_rounds"] * len(picked) / max(rounds, 1), 1)}
    result["results"].append(row)
    print(json.dumps({key: row[key] for key in ("query", "picks", "median_ms", "pass_ms", "loop_all_rounds_upper_estimate_ms")}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
