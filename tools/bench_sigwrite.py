"""Bulk save of a SketchSet (csrc/sigwrite.hpp) at full size on one GPU: the sets are generated in HBM, written as .zip by
SketchSetWriter, and the stages timed by the library's own counters (smgpu_sigwrite_stats).

    python tools/bench_sigwrite.py                     # the three shapes, medians of 7, -> profiles/sigwrite_bench.json
    python tools/bench_sigwrite.py --reps 3 --c5-rows 20000 --read-rows 200000 --big-hashes 1000000

Shapes: `c5` 100,000 rows x 5,000 hashes (BASELINE config C5's database), `reads` 10^6 rows of 0 .. 50 hashes (--singleton
sketches of reads), `big` one row of 10^7 hashes.  Hashes are uniform below max_hash(scaled = 1000), ascending in every row.
"Today's way" -- set.signature(r) -> save_signatures_to_json(compression = 1) -> zipfile, one Python object and one host sketch
per row -- is timed on the first rows of the same set in the same process, alternating with the device writer on the same
rows.  Also measures the size condition of tests/test_gpu_sigwrite.py (member against zlib level 1 + 18 bytes)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time
import zipfile
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sourmash_amd as sm  # noqa: E402
from sourmash_amd._lowlevel import lib  # noqa: E402
from sourmash_amd.index import SketchSet, SketchSetWriter  # noqa: E402

MAX_HASH = (1 << 64) // 1000
STAGES = ["lengths_ms", "md5_ms", "text_ms", "crc_ms", "pack_ms", "d2h_ms", "file_write_ms"]
COUNTS = ["rows", "hashes", "text_bytes", "bytes_written", "md5_host_rows"]


def stats(reset=True):
    out = (C.c_double * 12)()
    lib.smgpu_sigwrite_stats(out, 1 if reset else 0)
    return dict(zip(STAGES + COUNTS, list(out)))


def uniform_rows(n_rows, per_row, dev, gen):
    "n_rows x per_row ascending uniform hashes, as a CSR"
    rows_per_chunk = max(1, (1 << 26) // per_row)
    parts = []
    for r0 in range(0, n_rows, rows_per_chunk):
        m = torch.randint(1, MAX_HASH, (min(rows_per_chunk, n_rows - r0), per_row), dtype=torch.int64, device=dev, generator=gen)
        parts.append(torch.sort(m, dim=1).values.reshape(-1))
    hashes = torch.cat(parts)
    offsets = torch.arange(0, n_rows + 1, dtype=torch.int64, device=dev) * per_row
    return hashes, offsets


def read_rows(n_rows, max_per_row, dev, gen):
    "n_rows rows of 0 .. max_per_row ascending uniform hashes"
    counts = torch.randint(0, max_per_row + 1, (n_rows,), dtype=torch.int64, device=dev, generator=gen)
    m = torch.sort(torch.randint(1, MAX_HASH, (n_rows, max_per_row), dtype=torch.int64, device=dev, generator=gen), dim=1).values
    keep = torch.arange(max_per_row, device=dev)[None, :] < counts[:, None]
    offsets = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(counts, 0)
    return m[keep].contiguous(), offsets


def todays_way(sset, n, path):
    "one SourmashSignature and one gzip document per row, into a stored zip"
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as zf:
        for r in range(n):
            sig = sset.signature(r)
            zf.writestr(f"signatures/{sig.md5sum()}.sig.gz", sm.save_signatures_to_json([sig], compression=1))


def median_of(samples):
    return {k: statistics.median(s[k] for s in samples) for k in samples[0]}


def bench_shape(name, sset, reps, tmp, today_rows):
    res = {"rows": len(sset), "hashes": int(sset.total_hashes)}
    path = os.path.join(tmp, name + ".zip")
    runs = []
    for _ in range(reps):
        stats()
        t0 = time.perf_counter()
        sset.save(path)
        wall = (time.perf_counter() - t0) * 1e3
        s = stats()
        s["wall_ms"] = wall
        s["file_bytes"] = os.path.getsize(path)
        runs.append(s)
        os.unlink(path)
    res["device_writer"] = median_of(runs)
    res["device_writer"]["signatures_per_s"] = len(sset) / (res["device_writer"]["wall_ms"] / 1e3)
    if today_rows:
        n = min(today_rows, len(sset))
        sub = sset.subset(np.arange(n, dtype=np.uint64))
        dev_ms, host_ms = [], []
        for _ in range(reps):                                        # alternating, same rows, same process
            t0 = time.perf_counter()
            sub.save(path)
            dev_ms.append((time.perf_counter() - t0) * 1e3)
            os.unlink(path)
            t0 = time.perf_counter()
            todays_way(sub, n, path)
            host_ms.append((time.perf_counter() - t0) * 1e3)
            os.unlink(path)
        stats()
        res["first_rows"] = {"rows": n, "device_writer_ms": statistics.median(dev_ms), "todays_way_ms": statistics.median(host_ms),
                             "ratio": statistics.median(host_ms) / statistics.median(dev_ms)}
    return res


def size_condition(dev, gen):
    out = {}
    for n in (1000, 5000):
        hashes, offsets = uniform_rows(1, n, dev, gen)
        s = SketchSet.from_csr(hashes, offsets, ksize=31, scaled=1000, names=["NC_000913.3 Escherichia coli str. K-12 substr. MG1655, complete genome"],
                               filenames=["GCF_000005845.2_ASM584v2_genomic.fna.gz"])
        text = s.to_json()
        member = s.to_json(compression=1)
        limit = len(zlib.compress(text, 1)) + 18
        out[str(n)] = {"text_bytes": len(text), "member_bytes": len(member), "zlib1_plus_18": limit, "ratio": len(member) / limit}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--c5-rows", type=int, default=100_000)
    ap.add_argument("--read-rows", type=int, default=1_000_000)
    ap.add_argument("--big-hashes", type=int, default=10_000_000)
    ap.add_argument("--today-rows", type=int, default=10_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sigwrite_bench.json"))
    ap.add_argument("--tmp", default=None, help="directory for the files written (default: a temporary one)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20261019)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "shapes": {}}

    def flush():
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1, sort_keys=True)
            fh.write("\n")

    with tempfile.TemporaryDirectory(dir=args.tmp) as tmp:
        result["size_condition"] = size_condition(dev, gen)
        flush()
        shapes = [("reads", lambda: read_rows(args.read_rows, 50, dev, gen), args.today_rows),
                  ("big", lambda: uniform_rows(1, args.big_hashes, dev, gen), 0),
                  ("c5", lambda: uniform_rows(args.c5_rows, 5000, dev, gen), args.today_rows)]
        for name, make, today_rows in shapes:
            hashes, offsets = make()
            n = offsets.numel() - 1
            names = [f"read{i}" for i in range(n)] if name == "reads" else None
            sset = SketchSet.from_csr(hashes, offsets, ksize=31, scaled=1000, names=names, filenames=["reads.fq.gz"] * n if names else None)
            del hashes, offsets
            torch.cuda.empty_cache()
            sset.save(os.path.join(tmp, "warm.zip"))                 # first use: the arena's blocks, the pinned ring, the page cache
            os.unlink(os.path.join(tmp, "warm.zip"))
            result["shapes"][name] = bench_shape(name, sset, args.reps, tmp, today_rows)
            print(name, json.dumps(result["shapes"][name], sort_keys=True), flush=True)
            flush()
            del sset
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
