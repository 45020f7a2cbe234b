"""Per-record sketching throughput (csrc/sketch_records.hip) on resident synthetic DNA: records of 150, 10^4 and 10^7 bases at
k = 21 / 31 / 51, scaled = 1000.  Timed in one process, alternating: the (hash, position) kernel alone, the whole call (kernel +
assign + sort + offsets, DeviceSketcher.sketch_records) and the sketch kernel alone (DeviceSketcher.kernel_only) on the same
buffer; medians of `reps` runs after a warm-up.  Then end to end: a FASTA of 1 kb records through sketch_file(singleton=True)
against the record-by-record route (sketch_records(read_records(path), singleton=True): what sketch_file(singleton=True) ran
before the one-pass path existed), at k = 31, scaled = 100.
python tools/bench_singleton.py [bases=4e9] [reps=5] [out.json]   -> one JSON line (also written to out.json)"""
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from sourmash_amd import device as smd  # noqa: E402
from sourmash_amd import sketch as sms  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 4_000_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else None


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def med(xs):
    return statistics.median(xs)


out = {"bases": n, "reps": reps, "scaled": 1000, "runs": []}
for record_len in (150, 10_000, 10_000_000):
    seq = smd.synth_dna(n, seed=42, record_len=record_len)
    n_records = n // (record_len + 1)
    starts = torch.arange(n_records + 1, dtype=torch.int64, device="cuda") * (record_len + 1)
    for k in (21, 31, 51):
        sk = smd.DeviceSketcher(k, 1000)
        cap = sk.capacity_for(n)
        a, b = torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int64, device="cuda")
        count = torch.zeros(1, dtype=torch.int64, device="cuda")

        def pairs():
            count.zero_()
            sk.records_kernel_only(seq, a, b, count)

        def plain():
            count.zero_()
            sk.kernel_only(seq, a, count)

        whole = lambda: sk.sketch_records(seq, starts)      # noqa: E731
        pairs(); plain(); hashes, offsets = whole()          # warm-up
        t_pairs, t_plain, t_whole = [], [], []
        for _ in range(reps):
            t_pairs.append(timed(pairs)[0])
            kept_pairs = int(count.item())
            t_plain.append(timed(plain)[0])
            assert int(count.item()) == kept_pairs, "the two kernels keep different numbers of hashes"
            t_whole.append(timed(whole)[0])
        out["runs"].append({
            "record_len": record_len, "n_records": n_records, "k": k, "kept_pairs": kept_pairs, "entries": int(hashes.numel()),
            "pairs_kernel_Gbase_per_s": round(n / med(t_pairs) / 1e9, 2), "sketch_kernel_Gbase_per_s": round(n / med(t_plain) / 1e9, 2),
            "kernel_ratio": round(med(t_plain) / med(t_pairs), 3),
            "whole_call_Gbase_per_s": round(n / med(t_whole) / 1e9, 2), "whole_call_ms": round(med(t_whole) * 1e3, 2),
            "post_pass_share": round(max(0.0, 1.0 - med(t_pairs) / med(t_whole)), 3)})
        del a, b
    del seq, starts
    torch.cuda.empty_cache()

# end to end: FASTA files of 1 kb records
out["end_to_end"] = []
with tempfile.TemporaryDirectory() as d:
    for n_rec in (10_000, 100_000):
        text = smd.synth_dna(n_rec * 1001, seed=11, record_len=1000).cpu().numpy().tobytes()
        path = os.path.join(d, f"r{n_rec}.fa")
        with open(path, "wb") as f:
            f.write(b"".join(b">read%d\n" % i + rec + b"\n" for i, rec in enumerate(text.split(b"\n")) if rec))
        params = "k=31,scaled=100"
        sms.sketch_file(path, params, singleton=True)                          # warm-up
        t_new, sigs = timed(lambda: sms.sketch_file(path, params, singleton=True))

        def by_record():
            got = sms.sketch_records(list(sms.read_records(path)), params, filename=path, singleton=True)
            for s in got:
                len(s.minhash)                                                  # the queued records are hashed when looked at
            return got

        t_old, old = timed(by_record)
        assert len(sigs) == len(old) == n_rec
        for i in np.linspace(0, n_rec - 1, 50).astype(int):
            assert sigs[i].name == old[i].name and sigs[i].minhash.md5sum() == old[i].minhash.md5sum()
        out["end_to_end"].append({"records": n_rec, "record_len": 1000, "params": params, "one_pass_s": round(t_new, 4),
                                  "record_by_record_s": round(t_old, 4), "speedup": round(t_old / t_new, 2)})
line = json.dumps(out)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
