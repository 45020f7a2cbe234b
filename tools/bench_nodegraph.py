"""Nodegraph throughput, medians of alternated runs in one process with the input resident:
Nodegraph.add_device on synthetic DNA at k = 21 / 31 into 4 tables of 1e5 bits (the LDS form) and 4 tables of 1e9 bits (the
global form), HLL.add_device at p = 14 as the yardstick, and update_many / matches_many over 100,000 synthetic sketches of
about 5,000 hashes.  The tables are resident before each timed call (one add_device of a short prefix uploads them), so a
timed call is the kernel and its synchronisation.  Every run is checked: repeats give the same tables.
python tools/bench_nodegraph.py [bases=4e9] [reps=3] [sketches=100000]   -> one JSON line"""
import hashlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from sourmash_amd import MinHash  # noqa: E402
from sourmash_amd import device as smd  # noqa: E402
from sourmash_amd.hll import HLL  # noqa: E402
from sourmash_amd.index import SketchSet  # noqa: E402
from sourmash_amd.nodegraph import Nodegraph  # noqa: E402
from sourmash_amd.synth import synth_sketches_device  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 4_000_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
n_sk = int(float(sys.argv[3])) if len(sys.argv) > 3 else 100_000
seq = smd.synth_dna(n, seed=42, record_len=10_000_000)
prefix = seq[:4096]


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def digest(g):
    return hashlib.sha256(g.to_bytes(0)).hexdigest()[:16], g.n_occupied()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


out = {"bases": n, "reps": reps, "runs": []}
forms = {"lds": 100_000, "global": 1_000_000_000}
for k in (21, 31):
    rates = {f: [] for f in forms}
    rates["hll_p14"] = []
    ref = {}
    for _ in range(reps):           # alternated: LDS form, global form, HLL, then again
        for form, size in forms.items():
            g = Nodegraph(k, size, 4)
            g.add_device(prefix)    # uploads the tables
            rates[form].append(n / timed(lambda: g.add_device(seq)) / 1e9)
            d = digest(g)
            assert ref.setdefault(form, d) == d, "repeat runs disagree"
            ref[form + "_occupied"] = d[1]
            del g
        h = HLL.from_buffer(b"HLL" + bytes([1, 14, 50, k]) + bytes(1 << 14))
        rates["hll_p14"].append(n / timed(lambda: h.add_device(seq)) / 1e9)
    out["runs"].append({"k": k, "lds_4x1e5_Gbase_per_s": spread(rates["lds"]),
                        "global_4x1e9_Gbase_per_s": spread(rates["global"]), "hll_p14_Gbase_per_s": spread(rates["hll_p14"]),
                        "lds_vs_hll": round(statistics.median(rates["lds"]) / statistics.median(rates["hll_p14"]), 3),
                        "global_vs_hll": round(statistics.median(rates["global"]) / statistics.median(rates["hll_p14"]), 3),
                        "occupied": {f: ref[f + "_occupied"] for f in forms}})
del seq, prefix
torch.cuda.empty_cache()

# update_many / matches_many: n_sk sketches drawn from a shared pool (about 5,000 hashes each)
hs, offs = synth_sketches_device(n_sk, "cuda")
hs, offs = hs.cpu().numpy().view(np.uint64), offs.cpu().numpy()
mhs = []
for i in range(n_sk):
    mh = MinHash(0, 21, scaled=1)
    mh.add_many(hs[offs[i]:offs[i + 1]])
    mhs.append(mh)
sset = SketchSet(mhs)
total = int(offs[-1])
sk = {"sketches": n_sk, "hashes": total}
for form, size in forms.items():
    up, mt, ref = [], [], None
    for _ in range(reps):
        g = Nodegraph(21, size, 4)
        g.add_device(torch.zeros(64, dtype=torch.uint8, device="cuda"))   # uploads the tables
        up.append(total / timed(lambda: g.update_many(sset)) / 1e9)
        res = {}
        mt.append(total / timed(lambda: res.setdefault("m", g.matches_many(sset))) / 1e9)
        d = (digest(g), int(res["m"].sum()))
        assert ref is None or ref == d, "repeat runs disagree"
        ref = d
    sk[form] = {"update_many_Ghash_per_s": spread(up), "matches_many_Ghash_per_s": spread(mt), "occupied": ref[0][1],
                "matched": ref[1]}
out["sketches"] = sk
print(json.dumps(out))
