"""HyperLogLog throughput: HLL.add_device on resident synthetic DNA at k = 21 / 31 / 51 and p = 14 / 18, alternated in the
same process with the sketch kernel (DeviceSketcher, scaled = 1000) at the same k, plus HLL.add_file on plain and gzip FASTA.
Every run's registers are checked: repeats agree, and no register is below that of a run over a prefix of the input.
python tools/bench_hll.py [bases=4e9] [reps=3]   -> one JSON line"""
import gzip
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
from sourmash_amd.hll import HLL  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 4_000_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
seq = smd.synth_dna(n, seed=42, record_len=10_000_000)
prefix = seq[: n // 16]


def hll_for(k, p):
    return HLL.from_buffer(b"HLL" + bytes([1, p, 64 - p, k]) + bytes(1 << p))


def regs(h):
    return np.frombuffer(h.registers(), dtype=np.uint8)


def spread(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


out = {"bases": n, "reps": reps, "runs": []}
for k in (21, 31, 51):
    sk = smd.DeviceSketcher(k, 1000)
    sk.sketch(seq)
    for p in (14, 18):
        small = hll_for(k, p)
        small.add_device(prefix)
        ref = None
        hll_rate, sk_rate = [], []
        for _ in range(reps):
            h = hll_for(k, p)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h.add_device(seq)
            torch.cuda.synchronize()
            hll_rate.append(n / (time.perf_counter() - t0) / 1e9)
            r = regs(h)
            assert ref is None or np.array_equal(r, ref), "repeat runs disagree"
            assert (r >= regs(small)).all(), "a register is below the prefix run's"
            ref = r
            t0 = time.perf_counter()
            sk.sketch(seq)
            torch.cuda.synchronize()
            sk_rate.append(n / (time.perf_counter() - t0) / 1e9)
        out["runs"].append({"k": k, "p": p, "hll_Gbase_per_s": spread(hll_rate), "sketch_Gbase_per_s": spread(sk_rate),
                            "ratio": round(statistics.median(hll_rate) / statistics.median(sk_rate), 3),
                            "cardinality": h.cardinality()})

# add_file: 200 Mbase of FASTA, plain and gzip
fn = 200_000_000
text = smd.synth_dna(fn, seed=7, record_len=1_000_000).cpu().numpy().tobytes()
with tempfile.TemporaryDirectory() as d:
    body = b"".join(b">r%d\n" % i + rec + b"\n" for i, rec in enumerate(text.split(b"\n")) if rec)
    plain, gz = os.path.join(d, "x.fa"), os.path.join(d, "x.fa.gz")
    open(plain, "wb").write(body)
    with gzip.open(gz, "wb", compresslevel=1) as f:
        f.write(body)
    files = {}
    for name, path in (("fa", plain), ("fa.gz", gz)):
        rates, rr = [], None
        for _ in range(reps):
            h = hll_for(31, 14)
            t0 = time.perf_counter()
            _, bases = h.add_file(path)
            rates.append(bases / (time.perf_counter() - t0) / 1e9)
            assert rr is None or np.array_equal(regs(h), rr)
            rr = regs(h)
        files[name] = spread(rates)
    out["add_file_Gbase_per_s"] = files
print(json.dumps(out))
