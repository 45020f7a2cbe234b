"""K-mer finding throughput (csrc/sketch_find.hip) on resident synthetic DNA: 1 GB in records of 10^4 bases, k = 21 / 31 / 51,
scaled = 1000, queries of 5 x 10^3, 10^6 and 10^7 hashes of which about half occur in the buffer (as many as the buffer's own
sketch holds: about 10^6 at 1 GB, so the largest query has a tenth present).  Timed in one process, alternating: the find kernel
alone (KmerQuery.kernel_only), records_dna_kernel alone on the same buffer (DeviceSketcher.records_kernel_only: the yardstick --
the same walk, every kept pair written) and the whole KmerQuery.find (kernel + assign + sort + offsets + text + copies to the
host); medians of `reps` runs after a warm-up.  ratio = records kernel time / find kernel time (1: the same rate).
python tools/bench_find.py [bases=1e9] [reps=7] [out.json]   -> one JSON line (also written to out.json)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import sourmash_amd as sm  # noqa: E402
from sourmash_amd import device as smd  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
out_path = sys.argv[3] if len(sys.argv) > 3 else None
RECORD_LEN, SCALED = 10_000, 1000


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def med(xs):
    return statistics.median(xs)


seq = smd.synth_dna(n, seed=42, record_len=RECORD_LEN)
n_records = n // (RECORD_LEN + 1)
starts = torch.arange(n_records + 1, dtype=torch.int64, device="cuda") * (RECORD_LEN + 1)
out = {"bases": n, "reps": reps, "scaled": SCALED, "record_len": RECORD_LEN, "n_records": n_records, "runs": []}
rng = np.random.default_rng(5)
for k in (21, 31, 51):
    sk = smd.DeviceSketcher(k, SCALED)
    own = sk.sketch(seq).cpu().numpy().view(np.uint64).copy()                     # the buffer's sketch, sorted
    cap = sk.capacity_for(n)
    a, b = torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    for size in (5_000, 1_000_000, 10_000_000):
        present = rng.permutation(own)[:min(size // 2, len(own))]
        absent = rng.integers(1, sk.max_hash, size=size - len(present), dtype=np.uint64, endpoint=True)
        mh = sm.MinHash(0, k, scaled=SCALED)
        mh.add_many(np.unique(np.concatenate([present, absent])))
        query = sm.KmerQuery([mh])
        del mh

        def find_kernel():
            count.zero_()
            query.kernel_only(seq, a, b, count)

        def records_kernel():
            count.zero_()
            sk.records_kernel_only(seq, a, b, count)

        whole = lambda: query.find(seq, starts)                   # noqa: E731
        find_kernel(); records_kernel(); m = whole()              # warm-up (the first find puts the query on the device)
        t_find, t_rec, t_whole = [], [], []
        for _ in range(reps):
            t_find.append(timed(find_kernel)[0])
            matched = int(count.item())
            t_rec.append(timed(records_kernel)[0])
            kept = int(count.item())
            t_whole.append(timed(whole)[0])
        assert matched <= kept and len(m) <= matched
        out["runs"].append({
            "k": k, "query_hashes": len(query), "query_hashes_present": int(len(present)), "kept_pairs": kept, "matched_pairs": matched,
            "rows": len(m), "find_kernel_Gbase_per_s": round(n / med(t_find) / 1e9, 2),
            "records_kernel_Gbase_per_s": round(n / med(t_rec) / 1e9, 2), "ratio": round(med(t_rec) / med(t_find), 3),
            "find_kernel_ms": [round(t * 1e3, 3) for t in sorted(t_find)], "records_kernel_ms": [round(t * 1e3, 3) for t in sorted(t_rec)],
            "whole_find_ms": round(med(t_whole) * 1e3, 2), "whole_find_Gbase_per_s": round(n / med(t_whole) / 1e9, 2)})
        del query, m
    del a, b
line = json.dumps(out)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
