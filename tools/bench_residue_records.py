"""Per-record protein sketching throughput (csrc/protein_records.hip).

1. Resident input, pass only: a residue buffer of `residues` bytes without separators (protein input in records of 300) and one
   with a 0xFF after every 3,333 residues (the six segments of translated records of 10^4 bases), k = 10 / 16 / 42, scaled = 200.
   Timed in one process, alternating: the (hash, start) kernel and the hash-only kernel of the record-by-record route
   (residue_windows_launch) on the same buffer, then the whole call (DeviceSketcher.sketch_records: residues or translation,
   kernel, assign, sort, offsets) on the input those buffers stand for; medians of `reps` runs after a warm-up.
2. Whole call: a generated proteome of each of `records` records of 50 .. 600 residues through sketch_file(singleton=True)
   against the record-by-record route (sketch_records(read_records(path), singleton=True): what sketch_file(singleton=True) ran
   before the one-pass path existed), at protein k = 10, scaled = 200.
python tools/bench_residue_records.py [residues=1e9] [reps=7] [records=5000,500000] [out.json]   -> one JSON line (also written to out.json)"""
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

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
file_records = [int(x) for x in sys.argv[3].split(",") if x] if len(sys.argv) > 3 else [5_000, 500_000]
out_path = sys.argv[4] if len(sys.argv) > 4 else None
SCALED = 200
AMINO = torch.tensor(list(b"ACDEFGHIKLMNPQRSTVWY"), dtype=torch.uint8, device="cuda")
BASES = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def med(xs):
    return statistics.median(xs)


def letters(alphabet, count, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty(count, dtype=torch.uint8, device="cuda")
    step = 1 << 27
    for at in range(0, count, step):
        m = min(step, count - at)
        out[at:at + m] = alphabet[torch.randint(0, alphabet.numel(), (m,), device="cuda", generator=g)]
    return out


out = {"residues": n, "reps": reps, "scaled": SCALED, "runs": []}
for flavour in ("protein_records_of_300", "translated_records_of_10000"):
    translated = flavour.startswith("translated")
    aa = letters(AMINO, n // 8 * 8, 42)
    n_dev = None
    if translated:
        aa[3333::3334] = 0xff
        n_dev = torch.tensor([aa.numel()], dtype=torch.int64, device="cuda")
        n_in = n // 2                                           # bases that translate into about n residues
        seq = letters(BASES, n_in, 43)
        starts = torch.arange(n_in // 10_000 + 1, dtype=torch.int64, device="cuda") * 10_000
    else:
        seq = aa
        starts = torch.arange(aa.numel() // 300 + 1, dtype=torch.int64, device="cuda") * 300
    for k in (10, 16, 42):
        sk = smd.DeviceSketcher(k, SCALED)
        cap = int(aa.numel() / SCALED * 1.25) + 65_536
        a, b = torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, dtype=torch.int64, device="cuda")
        count = torch.zeros(1, dtype=torch.int64, device="cuda")

        def pairs():
            count.zero_()
            sk.residue_kernel_only(aa, a, b, count, n_dev=n_dev)

        def plain():
            count.zero_()
            sk.residue_kernel_only(aa, a, None, count)

        whole = lambda: sk.sketch_records(seq, starts, moltype="protein", is_protein=not translated)      # noqa: E731
        pairs(); plain(); hashes, offsets = whole()          # warm-up
        t_pairs, t_plain, t_whole = [], [], []
        for _ in range(reps):
            t_pairs.append(timed(pairs)[0])
            kept_pairs = int(count.item())
            t_plain.append(timed(plain)[0])
            kept_plain = int(count.item())
            t_whole.append(timed(whole)[0])
        # without separators the hash-only kernel skips nothing either: the counts agree; with them both skip the same windows
        assert kept_pairs == kept_plain, "the two kernels keep different numbers of hashes"
        out["runs"].append({
            "input": flavour, "n_records": int(starts.numel() - 1), "k": k, "kept_pairs": kept_pairs, "entries": int(hashes.numel()),
            "pairs_kernel_Gwindow_per_s": round(aa.numel() / med(t_pairs) / 1e9, 2),
            "hash_only_kernel_Gwindow_per_s": round(aa.numel() / med(t_plain) / 1e9, 2),
            "kernel_ratio": round(med(t_plain) / med(t_pairs), 3),
            "whole_call_ms": round(med(t_whole) * 1e3, 2), "whole_call_input_GB_per_s": round(seq.numel() / med(t_whole) / 1e9, 2)})
        del a, b
    del aa, seq, starts
    torch.cuda.empty_cache()

# whole call: generated proteomes
out["whole_call"] = []
with tempfile.TemporaryDirectory() as d:
    rng = np.random.default_rng(11)
    amino = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    for n_rec in file_records:
        lens = rng.integers(50, 601, size=n_rec)
        text = amino[rng.integers(0, 20, size=int(lens.sum()))].tobytes()
        ends = np.cumsum(lens)
        path = os.path.join(d, f"p{n_rec}.faa")
        with open(path, "wb") as f:
            f.write(b"".join(b">protein%d\n" % i + text[e - m:e] + b"\n" for i, (e, m) in enumerate(zip(ends.tolist(), lens.tolist()))))
        params = f"protein,k=10,scaled={SCALED}"
        kw = dict(singleton=True, moltype="protein", input_is_protein=True)
        sms.sketch_file(path, params, **kw)                                     # warm-up
        t_new, sigs = timed(lambda: sms.sketch_file(path, params, **kw))

        def by_record():
            got = sms.sketch_records(list(sms.read_records(path)), params, filename=path, **kw)
            for s in got:
                len(s.minhash)                                                  # the queued records are hashed when looked at
            return got

        t_old, old = timed(by_record)
        assert len(sigs) == len(old) == n_rec
        for i in np.linspace(0, n_rec - 1, 50).astype(int):
            assert sigs[i].name == old[i].name and sigs[i].minhash.md5sum() == old[i].minhash.md5sum()
        out["whole_call"].append({"records": n_rec, "residues": int(lens.sum()), "params": params, "one_pass_s": round(t_new, 4),
                                  "record_by_record_s": round(t_old, 4), "speedup": round(t_old / t_new, 2)})
line = json.dumps(out)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
