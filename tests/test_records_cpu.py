"""CPU checks of per-record sketching (csrc/sketch_records.hip): the C interface, the rule that assigns a k-mer to a record and
the packed / wide decision of the sort, both compiled for the host, and the Python entry points without a device.  None of this
needs a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sourmash_amd
from sourmash_amd._lowlevel import lib
from sourmash_amd.minhash import _get_max_hash_for_scaled

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")

PROTOTYPES = [
    "uint64_t smgpu_sketch_records_workspace_bytes(uint64_t pair_capacity, uint64_t n_records);",
    "uint64_t smgpu_sketch_records_raw(const uint8_t *d_seq, uint64_t len, const uint64_t *d_starts, uint64_t n_records, "
    "uint32_t ksize, uint64_t seed, uint64_t max_hash, uint64_t *d_hashes, uint64_t *d_abunds, uint64_t capacity, "
    "uint64_t *d_offsets, uint64_t *d_result, void *d_workspace, uint64_t workspace_bytes, void *stream);",
    "void smgpu_sketch_records_kernel_raw(const uint8_t *d_seq, uint64_t len, uint32_t ksize, uint64_t seed, uint64_t max_hash, "
    "uint64_t *d_hashes, uint64_t *d_positions, uint64_t capacity, uint64_t *d_count, void *stream);",
    "SmgpuSketchSet *smgpu_sketchset_sketch_records(const uint8_t *d_seq, uint64_t len, const uint64_t *d_starts, "
    "uint64_t n_records, uint32_t ksize, uint64_t seed, uint64_t scaled);",
    "SmgpuSketchSet *smgpu_sketchset_sketch_file(const char *path, uint32_t ksize, uint64_t seed, uint64_t scaled);",
    "SourmashSignature **smgpu_sketch_file_singleton(const char *path, const SourmashComputeParameters *params, uintptr_t *n);",
]


def _norm(s):
    return " ".join(s.replace("( ", "(").replace(" )", ")").split())


def test_prototypes_declared_and_exported():
    with open(os.path.join(ROOT, "include", "sourmash_amd.h")) as f:
        header = _norm(f.read())
    so = C.CDLL(os.path.join(ROOT, "sourmash_amd", "libsourmash_amd.so"))
    assert len(PROTOTYPES) == 6
    for p in PROTOTYPES:
        assert _norm(p) in header, p
        name = p.split("(")[0].split()[-1].lstrip("*")
        assert hasattr(so, name), name


# ---- the two rules, compiled for the host -----------------------------------------------------------------------------------
SRC = os.path.join(HERE, "native", "records_core_emul.cpp")
HDR = os.path.join(ROOT, "sourmash_amd", "csrc", "records_core.hpp")


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("records_core") / "librecords_core_emul.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", so_path, SRC])
    so = C.CDLL(so_path)
    so.emul_rec_assign.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    so.emul_rec_packed.argtypes = [C.c_uint64, C.c_uint64]
    so.emul_rec_hash_bits.argtypes = [C.c_uint64]
    assert os.path.exists(HDR)
    return so


def assign(emul, starts, pos, k):
    starts = np.asarray(starts, dtype=np.uint64)
    pos = np.asarray(pos, dtype=np.uint64)
    out = np.zeros(len(pos), dtype=np.int64)
    emul.emul_rec_assign(starts.ctypes.data, len(starts) - 1, pos.ctypes.data, len(pos), k, out.ctypes.data)
    return out.tolist()


def assign_py(starts, pos, k):
    "the rule written out: the last record starting at or before pos, if the k-mer ends inside it"
    n = len(starts) - 1
    if n == 0 or pos < starts[0]:
        return -1
    r = max(i for i in range(n + 1) if starts[i] <= pos)
    if r >= n or pos + k > starts[r + 1]:
        return -1
    return r


def test_assign_rule_cases(emul):
    k = 5
    # records: [10, 30), an empty one at 30, [30, 42), the last one [42, 50) ending at len = 50
    starts = [10, 30, 30, 42, 50]
    assert assign(emul, starts, [0, 9], k) == [-1, -1]                 # in front of starts[0]
    assert assign(emul, starts, [10, 25], k) == [0, 0]                 # first and last full k-mer of record 0
    assert assign(emul, starts, [26, 29], k) == [-1, -1]               # the k-mers that cross into the next record
    assert assign(emul, starts, [30, 37], k) == [2, 2]                 # the empty record 1 owns nothing: record 2 starts there
    assert assign(emul, starts, [38], k) == [-1]
    assert assign(emul, starts, [42, 45], k) == [3, 3]                 # the last record ends at len: its last k-mer ends at 50
    assert assign(emul, starts, [46, 49, 50, 51, 2**40], k) == [-1] * 5
    assert assign(emul, starts, [45], 1) == [3] and assign(emul, starts, [49], 1) == [3]
    # two touching records, no separator byte: k - 1 k-mers are lost to the boundary
    assert assign(emul, [0, 8, 16], list(range(16)), 3) == [0] * 6 + [-1] * 2 + [1] * 6 + [-1] * 2
    # no records at all
    assert assign(emul, [7], [0, 7, 8], 1) == [-1, -1, -1]


def test_assign_rule_matches_python(emul):
    rng = np.random.default_rng(5)
    for trial in range(50):
        n = int(rng.integers(1, 12))
        starts = np.sort(rng.integers(0, 80, size=n + 1))
        if trial % 3 == 0:
            starts[n // 2:] = np.maximum(starts[n // 2:], starts[n // 2])      # more equal starts: empty records
        starts = starts.tolist()
        for k in (1, 2, 7, 31):
            pos = list(range(0, 90))
            assert assign(emul, starts, pos, k) == [assign_py(starts, p, k) for p in pos], (starts, k)


def test_packed_or_wide(emul):
    """The packed form needs bits(n_records - 1) + bits(max_hash) <= 64.  max_hash at scaled = 1000 is 18446744073709552, which
    is above 2^54 and so has 55 significant bits: 9 bits are left for the record number and the line lies between 512 and 513
    records (1,024 records would need 10 + 55 = 65 bits; no 64-bit key tells 1,024 x max_hash pairs apart)."""
    mh1000 = _get_max_hash_for_scaled(1000)
    assert mh1000 == 18446744073709552 and emul.emul_rec_hash_bits(mh1000) == 55
    assert emul.emul_rec_hash_bits(0) == 64 and emul.emul_rec_hash_bits(_get_max_hash_for_scaled(1)) == 64
    assert emul.emul_rec_packed(1, mh1000) and emul.emul_rec_packed(2, mh1000) and emul.emul_rec_packed(512, mh1000)
    assert not emul.emul_rec_packed(513, mh1000)
    assert not emul.emul_rec_packed(1025, mh1000) and not emul.emul_rec_packed(100_000, mh1000)
    # scaled = 1: every hash bit counts, one record is packed, two are wide
    assert emul.emul_rec_packed(1, _get_max_hash_for_scaled(1)) and not emul.emul_rec_packed(2, _get_max_hash_for_scaled(1))
    assert emul.emul_rec_packed(1, 0) and not emul.emul_rec_packed(2, 0)
    # whatever is packed is lossless: the largest key fits 64 bits
    for scaled in (1, 2, 10, 100, 1000, 10**6):
        mh = _get_max_hash_for_scaled(scaled)
        for n in (1, 2, 3, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2**20, 2**32 - 2):
            hbits = mh.bit_length()
            assert bool(emul.emul_rec_packed(n, mh)) == ((n - 1).bit_length() + hbits <= 64), (scaled, n)
            if emul.emul_rec_packed(n, mh):
                assert (((n - 1) << hbits) | mh) < 2**64


# ---- without a device ---------------------------------------------------------------------------------------------------------
def test_entry_points_raise_without_gpu(tmp_path):
    if sourmash_amd.gpu_available():
        pytest.skip("a GPU is present: the calls succeed (covered by tests/test_gpu_records.py)")
    from sourmash_amd.exceptions import SourmashError
    from sourmash_amd.index import SketchSet
    from sourmash_amd.sketch import sketch_file
    from sourmash_amd.device import DeviceSketcher
    fa = tmp_path / "two.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n>b\nTTTTACGTACGGGGTACGTACGTACCCCGTACGTAC\n")
    with pytest.raises(SourmashError, match="no HIP device"):
        SketchSet.sketch_file(str(fa), ksize=21, scaled=1)
    with pytest.raises(SourmashError, match="no HIP device"):
        sketch_file(str(fa), "k=21,scaled=1", singleton=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        DeviceSketcher(ksize=21, scaled=1)
    with pytest.raises(RuntimeError, match="HIP device"):
        SketchSet.sketch_records(None, None, ksize=21, scaled=1)
    lib.sourmash_err_clear()
    assert lib.smgpu_sketchset_sketch_records(None, 0, None, 0, 21, 42, 1000) is None
    assert lib.sourmash_err_get_last_code() != 0
