#!/usr/bin/env python3
"""Set algebra on a resident collection: SketchSet.subtract / intersect / merge (csrc/setops.hip) against the loop over MinHash objects
that a user of the package wrote before they existed -- set.minhash(r) for every row, the operation, SketchSet(results).

    python tools/bench_setops.py [--rows 100000] [--row-size 5000] [--other 3000000] [--groups 1000] [--reps 7] [--loop-rows 2000]
                                 [--time-limit 1100] [--out profiles/setops_bench.json]

Workloads, on the C5 family of synth.synth_gather_device (rows of about --row-size hashes, half of them from a shared million-hash pool):
  subtract        one sketch of --other hashes (the pool and strangers) taken from every row;
  intersect_rows  every row intersected with the row of the same number of a second set of the family;
  merge_union     the rows merged into --groups groups (row r in group r mod groups), min_rows = 1;
  merge_all       the same groups, min_rows = "all".
Each is timed twice -- the set-level call (host clock, the new set made) and the kernels alone through the raw entry on caller-owned
buffers (device events around the call) -- as medians of --reps runs after a warm-up, in one process.  THE LOOP RUNS ON THE FIRST
--loop-rows ROWS ONLY AND IS SCALED TO THE FULL ROW COUNT (rows / loop-rows): the full loop would take minutes per run.  Its results
are compared with the set-level call on the same rows before anything is timed.  ratio = scaled loop median / set-level median
(above 1: the one call wins).  For the filter the raw time is also given as bytes/s against 8 x (hashes read + hashes written).
Needs a GPU; stops itself after --time-limit seconds."""
import argparse
import ctypes as C
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
    ap.add_argument("--other", type=int, default=3_000_000)
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loop-rows", type=int, default=2000)
    ap.add_argument("--time-limit", type=int, default=1100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "setops_bench.json"))
    args = ap.parse_args()

    def out_of_time(*_):
        print(f"bench_setops: the time limit of {args.time_limit} s ran out", file=sys.stderr, flush=True)
        os._exit(3)
    signal.signal(signal.SIGALRM, out_of_time)
    signal.alarm(args.time_limit)

    import numpy as np
    import torch
    import sourmash_amd as sm
    from sourmash_amd._lowlevel import lib
    from sourmash_amd.synth import MAX_HASH_1000, splitmix63, synth_gather_device
    assert sm.gpu_available(), "no HIP device visible"
    dev = torch.device("cuda:0")
    n, reps, loop_rows = args.rows, args.reps, min(args.loop_rows, args.rows)
    n_groups = min(args.groups, n)
    pool, hashes, offsets = synth_gather_device(1_000_000, 2 * n, args.row_size, dev, row_lo=0, row_hi=n)
    a = sm.SketchSet.from_csr(hashes, offsets, ksize=31, scaled=1000)
    total = int(offsets[-1])
    _, hashes, offsets = synth_gather_device(1_000_000, 2 * n, args.row_size, dev, row_lo=n, row_hi=2 * n)
    b = sm.SketchSet.from_csr(hashes, offsets, ksize=31, scaled=1000)
    strangers = splitmix63(torch.arange(int(1.02 * max(args.other - len(pool), 0)) + 16, device=dev, dtype=torch.int64) + 99) % MAX_HASH_1000 + 1
    other_t = torch.unique(torch.cat([pool, strangers]))[:args.other].contiguous()
    other = sm.SketchSet.from_csr(other_t, torch.tensor([0, len(other_t)], dtype=torch.int64, device=dev), ksize=31, scaled=1000)
    other_mh = other.minhash(0)
    del hashes, offsets, strangers, other_t
    groups = np.arange(n, dtype=np.int64) % n_groups
    loop_groups = max(1, loop_rows * n_groups // n)                     # the loop's rows in groups of the same size
    loop_group_of = np.arange(loop_rows) % loop_groups
    head = a.subset(np.arange(loop_rows))
    head_b = b.subset(np.arange(loop_rows))
    stream = torch.cuda.current_stream().cuda_stream

    def csr_ptrs(s):
        h, o = C.c_void_p(), C.c_void_p()
        lib.smgpu_sketchset_device_csr(s._get_objptr(), C.byref(h), C.byref(o))
        return h.value, o.value

    def timed_raw(call):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        got = call()
        t1.record()
        torch.cuda.synchronize()
        assert lib.sourmash_err_get_last_code() == 0 and got != 2**64 - 1
        return t0.elapsed_time(t1), got

    def filter_raw(other_set, rowwise, keep_present):
        ah, ao = csr_ptrs(a)
        oh, oo = csr_ptrs(other_set)
        o_len = 0 if rowwise else other_set.total_hashes
        ws_bytes = int(lib.smgpu_setops_filter_workspace_bytes(n, total, o_len))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty(total + 8, dtype=torch.int64, device=dev)
        out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        res = torch.zeros(2, dtype=torch.int64, device=dev)
        return lambda: lib.smgpu_setops_filter_raw(ah, ao, n, total, oh, oo if rowwise else None, o_len, keep_present, 0, out.data_ptr(), total,
                                                   out_off.data_ptr(), res.data_ptr(), ws.data_ptr(), ws_bytes, stream), (ws, out, out_off, res)

    def merge_raw(need_all):
        ah, ao = csr_ptrs(a)
        d_groups = torch.from_numpy(groups.astype(np.int32)).to(dev)
        ws_bytes = int(lib.smgpu_setops_merge_workspace_bytes(total, n_groups))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty(total + 8, dtype=torch.int64, device=dev)
        out_off = torch.empty(n_groups + 1, dtype=torch.int64, device=dev)
        res = torch.zeros(2, dtype=torch.int64, device=dev)
        return lambda: lib.smgpu_setops_merge_raw(ah, ao, n, total, d_groups.data_ptr(), n_groups, None, need_all, MAX_HASH_1000, 0, out.data_ptr(),
                                                  out_off.data_ptr(), res.data_ptr(), ws.data_ptr(), ws_bytes, stream), (d_groups, ws, out, out_off, res)

    def merged_loop(rows, all_rows):
        accs = []
        for g in range(loop_groups):
            acc = None
            for r in np.flatnonzero(loop_group_of == g):
                mh = rows.minhash(int(r))
                if acc is None:
                    acc = mh.to_mutable()
                elif all_rows:
                    acc = acc.intersection(mh)
                else:
                    acc.merge(mh)
            accs.append(acc)
        return sm.SketchSet(accs)

    def filter_loop(rows, op):
        out = []
        for r in range(loop_rows):
            mh = rows.minhash(r)
            out.append(op(mh, r))
        return sm.SketchSet(out)

    def subtract_one(mh, r):
        mh = mh.to_mutable()
        mh.remove_many(other_mh)
        return mh

    workloads = [
        ("subtract", lambda: a.subtract(other), lambda: filter_raw(other, False, 0), lambda: filter_loop(head, subtract_one), lambda: head.subtract(other)),
        ("intersect_rows", lambda: a.intersect(b), lambda: filter_raw(b, True, 1), lambda: filter_loop(head, lambda mh, r: mh.intersection(head_b.minhash(r))),
         lambda: head.intersect(head_b)),
        ("merge_union", lambda: a.merge(groups), lambda: merge_raw(0), lambda: merged_loop(head, False), lambda: head.merge(loop_group_of)),
        ("merge_all", lambda: a.merge(groups, min_rows="all"), lambda: merge_raw(1), lambda: merged_loop(head, True),
         lambda: head.merge(loop_group_of, min_rows="all")),
    ]
    result = {"device": torch.cuda.get_device_name(0), "rows": n, "total_hashes": total, "other_hashes": other.total_hashes, "groups": n_groups,
              "reps": reps, "loop_rows": loop_rows,
              "what": "ms; set_call = the SketchSet method end to end (host clock, the new set made), raw = the kernels through the raw entry on "
                      "caller-owned buffers (device events around the call), loop = the loop over MinHash objects ON loop_rows ROWS, "
                      "loop_scaled = its median x rows / loop_rows; ratio = loop_scaled / set_call median (above 1: the one call wins)",
              "results": []}
    for name, set_call, make_raw, loop, head_call in workloads:
        # warm-up, and the comparison on the loop's rows
        want, got = loop(), head_call()
        agree = [int(x) for x in want.sizes] == [int(x) for x in got.sizes] and want.md5sums() == got.md5sums()
        del want, got
        out_set = set_call()
        out_hashes = out_set.total_hashes
        del out_set
        raw_call, keep = make_raw()
        _, raw_total = timed_raw(raw_call)
        assert raw_total == out_hashes, (name, raw_total, out_hashes)
        runs = {"set_call": [], "raw": [], "loop": []}
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out_set = set_call()
            runs["set_call"].append((time.perf_counter() - t0) * 1e3)
            del out_set
            runs["raw"].append(timed_raw(raw_call)[0])
        del raw_call, keep
        for _ in range(reps):
            t0 = time.perf_counter()
            res = loop()
            runs["loop"].append((time.perf_counter() - t0) * 1e3)
            del res
        med = {k: statistics.median(v) for k, v in runs.items()}
        scaled = med["loop"] * n / loop_rows
        entry = {"workload": name, "agree": bool(agree), "result_hashes": int(out_hashes),
                 "median_ms": {k: round(v, 3) for k, v in med.items()}, "loop_scaled_ms": round(scaled, 1),
                 "ratio_loop_scaled_over_set_call": round(scaled / med["set_call"], 2), "ratio_loop_scaled_over_raw": round(scaled / med["raw"], 2),
                 "runs_ms": {k: [round(x, 3) for x in v] for k, v in runs.items()}}
        if name in ("subtract", "intersect_rows"):
            entry["raw_bytes_per_s"] = round(8 * (total + out_hashes) / (med["raw"] * 1e-3), 1)
            entry["raw_bytes_rule"] = "8 x (hashes read + hashes written) / raw median"
        result["results"].append(entry)
        print(json.dumps({k: entry[k] for k in ("workload", "agree", "median_ms", "loop_scaled_ms", "ratio_loop_scaled_over_set_call")}), flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"bench_setops: wrote {args.out}", flush=True)


if __name__ == "__main__":
    main()
