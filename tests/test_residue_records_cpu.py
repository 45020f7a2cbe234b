"""CPU checks of per-record protein / dayhoff / hp sketching (csrc/protein_records.hip): the C interface, the rule for records
with explicit ends and the per-record translation layout, both compiled for the host, and the Python entry points without a
device.  None of this needs a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import sourmash_amd
from sourmash_amd._lowlevel import lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")

PROTOTYPES = [
    "uint64_t smgpu_sketch_residue_records_workspace_bytes(uint64_t pair_capacity, uint64_t n_records, uint64_t len, int32_t translate);",
    "uint64_t smgpu_sketch_residue_records_raw(const uint8_t *d_seq, uint64_t len, const uint64_t *d_starts, const uint64_t *d_ends, "
    "uint64_t n_records, uint32_t ksize, uint32_t hash_function, int32_t translate, uint64_t seed, uint64_t max_hash, "
    "uint64_t *d_hashes, uint64_t *d_abunds, uint64_t capacity, uint64_t *d_offsets, uint64_t *d_result, void *d_workspace, "
    "uint64_t workspace_bytes, void *stream);",
    "SmgpuSketchSet *smgpu_sketchset_sketch_residue_records(const uint8_t *d_seq, uint64_t len, const uint64_t *d_starts, "
    "const uint64_t *d_ends, uint64_t n_records, uint32_t ksize, uint32_t hash_function, int32_t translate, uint64_t seed, "
    "uint64_t scaled);",
    "SmgpuSketchSet *smgpu_sketchset_sketch_residue_file(const char *path, uint32_t ksize, uint32_t hash_function, int32_t translate, "
    "uint64_t seed, uint64_t scaled);",
    "void smgpu_residue_records_kernel_raw(const uint8_t *d_aa, uint64_t n, const uint64_t *d_n, uint32_t ksize, uint64_t seed, "
    "uint64_t max_hash, uint64_t *d_hashes, uint64_t *d_positions, uint64_t capacity, uint64_t *d_count, void *stream);",
    "SourmashSignature **smgpu_sketch_file_singleton_residues(const char *path, const SourmashComputeParameters *params, "
    "int32_t input_is_protein, uintptr_t *n);",
]


def _norm(s):
    return " ".join(s.replace("( ", "(").replace(" )", ")").split())


def test_prototypes_declared_and_exported():
    with open(os.path.join(ROOT, "include", "sourmash_amd.h")) as f:
        header = _norm(f.read())
    so = C.CDLL(os.path.join(ROOT, "sourmash_amd", "libsourmash_amd.so"))
    for p in PROTOTYPES:
        assert _norm(p) in header, p
        name = p.split("(")[0].split()[-1].lstrip("*")
        assert hasattr(so, name), name
        assert hasattr(lib, name), name


def test_workspace_grows_with_every_argument():
    ws = lib.smgpu_sketch_residue_records_workspace_bytes
    base = ws(1000, 10, 5000, 0)
    assert ws(2000, 10, 5000, 0) > base and ws(1000, 10, 50_000, 0) > base
    assert ws(1000, 10, 5000, 1) >= base + 5000 + 60                  # translated: two residues per base, six separators a record
    assert ws(1000, 1000, 5000, 1) > ws(1000, 10, 5000, 1)


# ---- the rules, compiled for the host -------------------------------------------------------------------------------------------
SRC = os.path.join(HERE, "native", "residue_records_emul.cpp")


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so_path = str(tmp_path_factory.mktemp("residue_records") / "libresidue_records_emul.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", so_path, SRC])
    so = C.CDLL(so_path)
    so.emul_rec_assign_ends.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
    so.emul_rec_ends_valid.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    so.emul_block_starts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    so.emul_block_starts.restype = C.c_uint64
    so.emul_translated_records_bound.argtypes = [C.c_uint64, C.c_uint64]
    so.emul_translated_records_bound.restype = C.c_uint64
    so.emul_translate_records.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
    return so


def assign(emul, starts, ends, pos, k):
    starts = np.asarray(starts, dtype=np.uint64)
    ends_a = None if ends is None else np.asarray(ends, dtype=np.uint64)
    pos = np.asarray(pos, dtype=np.uint64)
    out = np.zeros(len(pos), dtype=np.int64)
    emul.emul_rec_assign_ends(starts.ctypes.data, None if ends is None else ends_a.ctypes.data, len(starts) - 1, pos.ctypes.data, len(pos), k,
                              out.ctypes.data)
    return out


def assign_np(starts, ends, pos, k):
    "the rule restated: the last record starting at or before pos, if the window ends at or before that record's end"
    starts = np.asarray(starts, dtype=np.int64)
    n = len(starts) - 1
    pos = np.asarray(pos, dtype=np.int64)
    if n == 0:
        return np.full(len(pos), -1, dtype=np.int64)
    ends = starts[1:] if ends is None else np.asarray(ends, dtype=np.int64)
    r = np.searchsorted(starts, pos, side="right") - 1
    ok = (r >= 0) & (r < n)
    ok &= pos + k <= ends[np.clip(r, 0, n - 1)]
    return np.where(ok, r, -1)


def test_ends_rule_cases(emul):
    k = 5
    # records [10, 29) + gap byte 29, an empty one at 30 (end 30), [30, 41) + gap byte 41, the last one [42, 50)
    starts, ends = [10, 30, 30, 42, 50], [29, 30, 41, 50]
    a = lambda pos, kk=k: assign(emul, starts, ends, pos, kk).tolist()   # noqa: E731
    assert a([0, 9]) == [-1, -1]                                     # in front of starts[0]
    assert a([10, 24]) == [0, 0]                                     # first and last full window of record 0
    assert a([25]) == [-1]                                           # the window that ends on the gap byte
    assert assign(emul, starts, None, [25], k).tolist() == [0]       # ... which records that touch would keep
    assert a([26, 29]) == [-1, -1]
    assert a([30, 36]) == [2, 2] and a([37]) == [-1]
    assert a([42, 45]) == [3, 3] and a([46, 49, 50, 2**40]) == [-1] * 4
    assert a([28], 1) == [0] and a([29], 1) == [-1] and a([41], 1) == [-1] and a([49], 1) == [3]
    # ends None is the rule of touching records
    assert assign(emul, [0, 8, 16], None, list(range(16)), 3).tolist() == [0] * 6 + [-1] * 2 + [1] * 6 + [-1] * 2
    assert assign(emul, [7], None, [0, 7, 8], 1).tolist() == [-1, -1, -1]
    # a record's end must lie inside [starts[r], starts[r + 1]]
    s = np.asarray([100, 500, 1000], dtype=np.uint64)
    for e, want in (([100, 500], (1, 1)), ([500, 1000], (1, 1)), ([99, 900], (0, 1)), ([501, 1000], (0, 1)), ([500, 1001], (1, 0))):
        e = np.asarray(e, dtype=np.uint64)
        assert (emul.emul_rec_ends_valid(s.ctypes.data, e.ctypes.data, 0), emul.emul_rec_ends_valid(s.ctypes.data, e.ctypes.data, 1)) == want


def test_ends_rule_hand_placed_layout(emul):
    "records that begin or end at 7, 8, 9 and 2047, 2048, 2049, empty records, touching and with a gap byte"
    for k in (1, 7, 8, 9, 16, 79):
        lens = [1, 1, 2038, 1, 1, 0, 0, 1, k - 1, k, k + 1, 5000]
        for gaps in (False, True):
            starts, ends, at = [7], [], 7
            for n in lens:
                at += n
                ends.append(at)
                at += 1 if gaps else 0
                starts.append(at)
            pos = np.arange(0, at + 10)
            want = assign_np(starts, ends if gaps else None, pos, k)
            assert np.array_equal(assign(emul, starts, ends if gaps else None, pos, k), want), (k, gaps)
            if not gaps:
                assert starts[:6] == [7, 8, 9, 2047, 2048, 2049]


def test_ends_rule_matches_numpy_on_random_records(emul):
    rng = np.random.default_rng(9)
    done = 0
    while done < 10_000:
        n = int(rng.integers(1, 12))
        starts = np.sort(rng.integers(0, 200, size=n + 1))
        if done % 3 == 0:
            starts[n // 2:] = np.maximum(starts[n // 2:], starts[n // 2])      # more equal starts: empty records
        ends = np.asarray([rng.integers(starts[r], starts[r + 1] + 1) for r in range(n)])
        k = int(rng.choice([1, 2, 7, 10, 42, 79]))
        pos = rng.integers(0, 220, size=100)
        assert np.array_equal(assign(emul, starts, ends, pos, k), assign_np(starts, ends, pos, k)), (starts, ends, k)
        assert np.array_equal(assign(emul, starts, None, pos, k), assign_np(starts, None, pos, k)), (starts, k)
        done += 100


# ---- the per-record translation layout ----------------------------------------------------------------------------------------------
def translate_py(rec, hf):
    "the six segments of one record from the oracle's codon table, each followed by 0xFF"
    comp = {65: 84, 67: 71, 71: 67, 84: 65, 78: 78}
    up = bytes(rec).upper()
    rc = bytes(comp.get(c, 0) for c in reversed(up))
    dayhoff = {**dict.fromkeys("C", "a"), **dict.fromkeys("AGPST", "b"), **dict.fromkeys("DENQ", "c"), **dict.fromkeys("HKR", "d"),
               **dict.fromkeys("ILMV", "e"), **dict.fromkeys("FWY", "f"), "*": "*"}
    hp = {**dict.fromkeys("AFGILMPVWY", "h"), **dict.fromkeys("NCSTDERHKQ", "p"), "*": "*"}
    enc = (lambda a: a) if hf == 2 else (lambda a: dayhoff.get(a, "X")) if hf == 3 else (lambda a: hp.get(a, "X"))
    out = bytearray()
    for frame in range(3):
        for strand in (up, rc):
            for p in range(frame, len(strand) - 2, 3):
                out += enc(oracle.translate_codon(strand[p:p + 3])).encode()
            out.append(0xff)
    return bytes(out)


def test_translate_records_layout(emul):
    rng = np.random.default_rng(21)
    k = 10
    lens = [3 * k - 1, 3 * k, 3 * k + 1, 3 * k + 2, 3 * k + 3, 0, 1, 0, 2, 3, 4, 5, 6, 7, 8, 9, 4095, 4096, 4097, 300]
    for gaps in (False, True):
        parts, starts, ends, at = [b"TTACG"], [5], [], 5
        for n in lens:
            rec = bytearray(rng.choice(list(b"ACGT"), size=n).astype(np.uint8).tobytes())
            if n == 300:
                rec[30] = ord("N"); rec[61] = ord("n"); rec[92] = ord("N"); rec[120:124] = b"RYKM"; rec[150] = 0xff; rec[160] = ord(">")
                rec[200:260] = bytes(rec[200:260]).lower()
            parts.append(bytes(rec))
            at += n
            ends.append(at)
            if gaps:
                parts.append(b">")
                at += 1
            starts.append(at)
        seq = np.frombuffer(b"".join(parts), dtype=np.uint8)
        starts_a, ends_a = np.asarray(starts, dtype=np.uint64), np.asarray(ends, dtype=np.uint64)
        e_ptr = ends_a.ctypes.data if gaps else None
        n = len(lens)
        blocks = np.zeros(n + 1, dtype=np.uint64)
        total = emul.emul_block_starts(starts_a.ctypes.data, e_ptr, n, blocks.ctypes.data)
        for hf in (2, 3, 4):
            want = [translate_py(seq[starts[r]:ends[r]], hf) for r in range(n)]
            # block starts equal the prefix sum of what one record's layout gives, and stay below the bound
            assert np.array_equal(blocks, np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.uint64))
            assert total == blocks[n] <= emul.emul_translated_records_bound(len(seq), n)
            out = np.full((total + 7) // 8 * 8, 0xAA, dtype=np.uint8)
            block_of = np.zeros(total, dtype=np.uint64)
            emul.emul_translate_records(seq.ctypes.data, starts_a.ctypes.data, e_ptr, blocks.ctypes.data, n, hf, out.ctypes.data, block_of.ctypes.data)
            assert bytes(out[:total]) == b"".join(want)
            assert not out[total:].any()                              # the last word's tail is zero
            assert np.array_equal(block_of, np.repeat(np.arange(n, dtype=np.uint64), [len(w) for w in want]))
            assert all(w.endswith(b"\xff") and w.count(b"\xff") == 6 for w in want if 0xff not in want)


# ---- without a device ---------------------------------------------------------------------------------------------------------------
def test_entry_points_raise_without_gpu(tmp_path):
    if sourmash_amd.gpu_available():
        pytest.skip("a GPU is present: the calls succeed (covered by tests/test_gpu_residue_records.py)")
    from sourmash_amd.exceptions import SourmashError
    from sourmash_amd.index import SketchSet
    from sourmash_amd.sketch import sketch_file, sketch_file_to
    fa = tmp_path / "two.faa"
    fa.write_text(">a\nMKVLAAGIVGLLLAQWERTPPGHHDESTT\n>b\nPPGHHDESTTRRKLMNACMKVLAAGIV\n")
    with pytest.raises(SourmashError, match="no HIP device"):
        SketchSet.sketch_file(str(fa), ksize=10, scaled=1, moltype="protein", input_is_protein=True)
    with pytest.raises(SourmashError, match="no HIP device"):
        sketch_file(str(fa), "protein,k=10,scaled=1", singleton=True, moltype="protein", input_is_protein=True)
    with pytest.raises(SourmashError, match="no HIP device"):
        sketch_file(str(fa), "dayhoff,k=7,scaled=1", singleton=True, moltype="dayhoff")
    with pytest.raises(SourmashError, match="no HIP device"):
        sketch_file_to(str(fa), str(tmp_path / "out.zip"), "protein,k=10,scaled=1", moltype="protein", input_is_protein=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        SketchSet.sketch_records(None, None, ksize=10, scaled=1, moltype="protein", is_protein=True)
    lib.sourmash_err_clear()
    assert lib.smgpu_sketchset_sketch_residue_records(None, 0, None, None, 0, 10, 2, 0, 42, 1000) is None
    assert lib.sourmash_err_get_last_code() != 0
    lib.sourmash_err_clear()
