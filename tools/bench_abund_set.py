#!/usr/bin/env python3
"""Abundance sets: the value-moving forms of the SketchSet set algebra (csrc/setops.hip) against their flat forms on the same inputs,
and against the loop over MinHash objects that does the same without them.

    python tools/bench_abund_set.py [--rows 100000] [--row-size 5000] [--other 3000000] [--groups 1000] [--reps 7] [--loop-rows 2000]
                                    [--angular-rows 1000] [--time-limit 1100] [--out profiles/abund_set_bench.json] [--shapes-only]

The set is that of tools/bench_setops.py (the C5 family of synth.synth_gather_device) with a seeded abundance column: a function
of the hash, 1 .. 64.  Workloads, each as medians of --reps runs after a warm-up, in one process, host clock around the set-level call:
  inflate_one      the flat set inflated by one abundance sketch of --other hashes      (flat form: intersect with the same sketch)
  inflate_rows     the flat set inflated row by row by a second abundance set           (flat form: row-wise intersect)
  subtract_carry   the abundance set without the hashes of the one sketch              (flat form: subtract on the flat set)
  filter_abund     the abundance set cut to abundances 2 .. 40                          (no flat form: the flatten() copy is given)
  merge_sum        the abundance set merged into --groups groups, abundances summed     (flat form: merge of the flat set)
  count_rows       the flat set merged with count_rows=True                             (flat form: merge of the flat set)
  compare_angular  SketchSet.compare_angular() on --angular-rows rows against compare.angular_matrix over the same sketches as objects
ratio_abund_over_flat = abundance median / flat median.  THE LOOP OVER OBJECTS RUNS ON THE FIRST --loop-rows ROWS ONLY AND IS SCALED
TO THE FULL ROW COUNT; its results are compared (hashes and abundances, row by row) with the set-level call on the same rows before
anything is timed.  The bytes a form must move are computed from the shapes: a flat filter 8 x (hashes read + hashes written); the
carry adds 16 bytes a kept hash (one abundance read, one written); the take adds one scattered 8-byte read and one 8-byte write a kept
hash; the range reads 16 bytes a hash and writes 16 a kept one; the summing merge adds, per input hash, one gathered 8-byte read and
the two scans (8 in, 8 out each), and 8 bytes a kept hash.
--shapes-only: no GPU; writes the record with the byte rules and every time "not measured".  Stops itself after --time-limit seconds."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOT_MEASURED = "not measured"
WORKLOADS = ["inflate_one", "inflate_rows", "subtract_carry", "filter_abund", "merge_sum", "count_rows", "compare_angular"]


def byte_rules(name, total, kept, other):
    "the bytes the flat form moves, and what the abundance form adds, from the shapes (None where the result size is not known)"
    if kept is None:
        return {"flat_bytes": NOT_MEASURED, "abund_extra_bytes": NOT_MEASURED}
    if name in ("inflate_one", "inflate_rows"):
        return {"flat_bytes": 8 * (total + kept), "abund_extra_bytes": 16 * kept, "rule": "flat 8 x (read + written); + one scattered 8-byte read and one 8-byte write a kept hash"}
    if name == "subtract_carry":
        return {"flat_bytes": 8 * (total + kept), "abund_extra_bytes": 16 * kept, "rule": "flat 8 x (read + written); + 16 bytes a kept hash (one abundance read, one written)"}
    if name == "filter_abund":
        return {"flat_bytes": 16 * total, "abund_extra_bytes": 16 * total + 16 * kept,
                "rule": "flat: the flatten() copy, 8 read + 8 written a hash; range: 16 read a hash in the count and in the write mode, 16 written a kept hash"}
    if name == "merge_sum":
        return {"flat_bytes": NOT_MEASURED, "abund_extra_bytes": 8 * total + 4 * 8 * total + 8 * kept, "rule": "+ per input hash one gathered 8-byte read and two scans (8 in + 8 out each), + 8 bytes a kept hash; the flat merge's bytes are the sort's"}
    if name == "count_rows":
        return {"flat_bytes": NOT_MEASURED, "abund_extra_bytes": 8 * kept, "rule": "+ 8 bytes a kept hash (the run's length is already in a register)"}
    return {"flat_bytes": NOT_MEASURED, "abund_extra_bytes": NOT_MEASURED}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--row-size", type=int, default=5000)
    ap.add_argument("--other", type=int, default=3_000_000)
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loop-rows", type=int, default=2000)
    ap.add_argument("--angular-rows", type=int, default=1000)
    ap.add_argument("--time-limit", type=int, default=1100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "abund_set_bench.json"))
    ap.add_argument("--shapes-only", action="store_true")
    args = ap.parse_args()
    shape = {"rows": args.rows, "row_size": args.row_size, "other_hashes": args.other, "groups": min(args.groups, args.rows), "reps": args.reps,
             "loop_rows": min(args.loop_rows, args.rows), "angular_rows": min(args.angular_rows, args.rows)}
    what = ("ms, host clock around the set-level call; abund = the abundance form, flat = its flat form on the same inputs, loop = the loop over "
            "MinHash objects ON loop_rows ROWS, loop_scaled = its median x rows / loop_rows; ratio_abund_over_flat = abund / flat medians")
    if args.shapes_only:
        total = args.rows * args.row_size
        record = dict(shape, device=NOT_MEASURED, total_hashes_nominal=total, what=what, status=NOT_MEASURED,
                      flat_path_parent_vs_branch={"status": NOT_MEASURED, "how": "tools/bench_setops.py on the parent commit and on this one in one GPU call, "
                                                  "alternating; the margin is the spread of the parent against itself in that call"},
                      results=[dict(workload=w, agree=NOT_MEASURED, median_ms=NOT_MEASURED, ratio_abund_over_flat=NOT_MEASURED, loop_scaled_ms=NOT_MEASURED,
                                    bytes=dict(byte_rules(w, total, None, args.other), per_kept_hash={"inflate_one": 16, "inflate_rows": 16, "subtract_carry": 16,
                                                                                                      "filter_abund": 16, "merge_sum": 8, "count_rows": 8}.get(w, NOT_MEASURED)))
                               for w in WORKLOADS])
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
        print(f"bench_abund_set: wrote {args.out} (shapes only: nothing was measured)", flush=True)
        return

    def out_of_time(*_):
        print(f"bench_abund_set: the time limit of {args.time_limit} s ran out", file=sys.stderr, flush=True)
        os._exit(3)
    signal.signal(signal.SIGALRM, out_of_time)
    signal.alarm(args.time_limit)

    import numpy as np
    import torch
    import sourmash_amd as sm
    from sourmash_amd.compare import angular_matrix
    from sourmash_amd.synth import MAX_HASH_1000, splitmix63, synth_gather_device
    assert sm.gpu_available(), "no HIP device visible"
    dev = torch.device("cuda:0")
    n, reps, loop_rows, n_groups = args.rows, args.reps, shape["loop_rows"], shape["groups"]

    def abund_of(h):
        return (splitmix63(h) & 63) + 1                                  # seeded by the hash: 1 .. 64

    def both(hashes, offsets):
        return (sm.SketchSet.from_csr(hashes, offsets, ksize=31, scaled=1000),
                sm.SketchSet.from_csr(hashes, offsets, ksize=31, scaled=1000, abunds=abund_of(hashes).contiguous()))
    pool, hashes, offsets = synth_gather_device(1_000_000, 2 * n, args.row_size, dev, row_lo=0, row_hi=n)
    a_flat, a_ab = both(hashes, offsets)
    total = int(offsets[-1])
    _, hashes, offsets = synth_gather_device(1_000_000, 2 * n, args.row_size, dev, row_lo=n, row_hi=2 * n)
    b_flat, b_ab = both(hashes, offsets)
    strangers = splitmix63(torch.arange(int(1.02 * max(args.other - len(pool), 0)) + 16, device=dev, dtype=torch.int64) + 99) % MAX_HASH_1000 + 1
    other_t = torch.unique(torch.cat([pool, strangers]))[:args.other].contiguous()
    other_flat, other_ab = both(other_t, torch.tensor([0, len(other_t)], dtype=torch.int64, device=dev))
    other_mh, other_ab_mh = other_flat.minhash(0), other_ab.minhash(0)
    other_dict = other_ab_mh.hashes
    del hashes, offsets, strangers, other_t
    groups = np.arange(n, dtype=np.int64) % n_groups
    loop_groups = max(1, loop_rows * n_groups // n)
    loop_group_of = np.arange(loop_rows) % loop_groups
    head = np.arange(loop_rows)
    ha_flat, ha_ab, hb_ab = a_flat.subset(head), a_ab.subset(head), b_ab.subset(head)

    def abund_sketch(like, values):
        mh = like.copy_and_clear().to_mutable()
        mh.set_abundances(values)
        return mh

    def loop_inflate_one():
        out = []
        for r in range(loop_rows):
            mh = ha_flat.minhash(r)
            out.append(abund_sketch(other_ab_mh, {h: other_dict.get(h, 0) for h in mh.hashes}))      # (MinHash.inflate with the dictionary made once)
        return out

    def loop_inflate_rows():
        return [ha_flat.minhash(r).inflate(hb_ab.minhash(r)) for r in range(loop_rows)]

    def loop_subtract():
        out = []
        for r in range(loop_rows):
            mh = ha_ab.minhash(r).to_mutable()
            mh.remove_many(other_mh)
            out.append(mh)
        return out

    def loop_filter():
        out = []
        for r in range(loop_rows):
            mh = ha_ab.minhash(r)
            out.append(abund_sketch(mh, {h: v for h, v in mh.hashes.items() if 2 <= v <= 40}))
        return out

    def loop_merge(count):
        accs = []
        for g in range(loop_groups):
            acc = None
            for r in np.flatnonzero(loop_group_of == g):
                mh = ha_ab.minhash(int(r))
                if count:
                    mh = abund_sketch(mh, {h: 1 for h in mh.hashes})
                if acc is None:
                    acc = mh.to_mutable()
                else:
                    acc.merge(mh)
            accs.append(acc)
        return accs

    workloads = [
        ("inflate_one", lambda: a_flat.inflate(other_ab), lambda: a_flat.intersect(other_flat), loop_inflate_one, lambda: ha_flat.inflate(other_ab)),
        ("inflate_rows", lambda: a_flat.inflate(b_ab), lambda: a_flat.intersect(b_flat), loop_inflate_rows, lambda: ha_flat.inflate(hb_ab)),
        ("subtract_carry", lambda: a_ab.subtract(other_flat), lambda: a_flat.subtract(other_flat), loop_subtract, lambda: ha_ab.subtract(other_flat)),
        ("filter_abund", lambda: a_ab.filter_abund(2, 40), lambda: a_ab.flatten(), loop_filter, lambda: ha_ab.filter_abund(2, 40)),
        ("merge_sum", lambda: a_ab.merge(groups), lambda: a_flat.merge(groups), lambda: loop_merge(False), lambda: ha_ab.merge(loop_group_of)),
        ("count_rows", lambda: a_flat.merge(groups, count_rows=True), lambda: a_flat.merge(groups), lambda: loop_merge(True),
         lambda: ha_flat.merge(loop_group_of, count_rows=True)),
    ]
    result = dict(shape, device=torch.cuda.get_device_name(0), total_hashes=total, what=what,
                  flat_path_parent_vs_branch={"status": NOT_MEASURED, "how": "tools/bench_setops.py on the parent commit and on this one in one GPU call, alternating"},
                  results=[])

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, out

    for name, abund_call, flat_call, loop, head_call in workloads:
        want, got = loop(), head_call()                                  # warm-up, and the comparison on the loop's rows
        agree = len(want) == len(got) and all(got.minhash(r).hashes == want[r].hashes for r in range(len(want)))
        del want, got
        kept = abund_call().total_hashes
        flat_call()
        runs = {"abund": [], "flat": [], "loop": []}
        for _ in range(reps):
            runs["abund"].append(timed(abund_call)[0])
            runs["flat"].append(timed(flat_call)[0])
        for _ in range(reps):
            runs["loop"].append(timed(loop)[0])
        med = {k: statistics.median(v) for k, v in runs.items()}
        scaled = med["loop"] * n / loop_rows
        entry = {"workload": name, "agree": bool(agree), "result_hashes": int(kept), "median_ms": {k: round(v, 3) for k, v in med.items()},
                 "ratio_abund_over_flat": round(med["abund"] / med["flat"], 3), "loop_scaled_ms": round(scaled, 1),
                 "ratio_loop_scaled_over_abund": round(scaled / med["abund"], 2), "bytes": byte_rules(name, total, int(kept), other_flat.total_hashes),
                 "runs_ms": {k: [round(x, 3) for x in v] for k, v in runs.items()}}
        result["results"].append(entry)
        print(json.dumps({k: entry[k] for k in ("workload", "agree", "median_ms", "ratio_abund_over_flat", "loop_scaled_ms")}), flush=True)

    m = shape["angular_rows"]
    sub = a_ab.subset(np.arange(m))
    objects = [sub.minhash(r) for r in range(m)]
    agree = bool(np.array_equal(sub.compare_angular(), angular_matrix(objects)))
    runs = {"set": [], "objects": []}
    for _ in range(reps):
        runs["set"].append(timed(sub.compare_angular)[0])
        runs["objects"].append(timed(lambda: angular_matrix(objects))[0])
    med = {k: statistics.median(v) for k, v in runs.items()}
    entry = {"workload": "compare_angular", "agree": agree, "rows": m, "median_ms": {k: round(v, 3) for k, v in med.items()},
             "ratio_objects_over_set": round(med["objects"] / med["set"], 2), "runs_ms": {k: [round(x, 3) for x in v] for k, v in runs.items()}}
    result["results"].append(entry)
    print(json.dumps({k: entry[k] for k in ("workload", "agree", "median_ms", "ratio_objects_over_set")}), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"bench_abund_set: wrote {args.out}", flush=True)


if __name__ == "__main__":
    main()
