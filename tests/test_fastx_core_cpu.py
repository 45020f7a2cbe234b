"""CPU check of the FASTA / FASTQ parser's rules (sourmash_amd/csrc/fastx_core.hpp compiled for the host) through an emulation of
fastx.hip's three kernels with lanes as loop indices (tests/native/fastx_emul.cpp), against the per-line reference and the cases
of tests/fastx_cases.py: whole files and files in pieces with the carry chained, the record-starts capacity, and once more as a
stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer.  No GPU needed."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle
import fastx_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "fastx_emul.cpp")
HDRS = [os.path.join(HERE, "..", "sourmash_amd", "csrc", "fastx_core.hpp")]
GUARD = 0xA5A5A5A5A5A5A5A5


def build(name, *flags):
    out = os.path.join(HERE, "native", name)
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(out) or os.path.getmtime(out) < newest:
        subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", *flags, "-o", out, SRC])
    return out


@pytest.fixture(scope="module")
def emul():
    lib = C.CDLL(build("libfastx_emul.so", "-O2", "-shared", "-fPIC"))
    lib.fastx_emul_piece.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.fastx_emul_pieces.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_uint64, C.c_void_p]

    def run(raw, fastq, cuts=None, cap=None, guard=0):
        "-> (bytes, starts[:min(cap, records)], kept, records, (state, ended on LF), the guard words behind the starts)"
        n = len(raw)
        carry = np.array([3 if fastq else 1, 1, 0, 0], dtype=np.uint8)
        out = np.zeros(n + 1, dtype=np.uint8)
        cap = n + 1 if cap is None else cap
        starts = np.full(cap + guard, GUARD, dtype=np.uint64)
        res = np.zeros(2, dtype=np.uint64)
        if cuts is None:
            lib.fastx_emul_piece(raw, n, fastq, carry.ctypes.data, out.ctypes.data, starts.ctypes.data, cap, res.ctypes.data)
        else:
            cuts = np.ascontiguousarray(cuts, dtype=np.uint64)
            lib.fastx_emul_pieces(raw, n, fastq, cuts.ctypes.data, len(cuts), carry.ctypes.data, out.ctypes.data, starts.ctypes.data, cap,
                                  res.ctypes.data)
        kept, recs = int(res[0]), int(res[1])
        return out[:kept].tobytes(), starts[:min(cap, recs)], kept, recs, (int(carry[0]), int(carry[1])), starts[min(cap, recs):]
    return run


def check(got, want, what):
    out, starts, kept, recs, carry, _ = got
    assert kept == want.kept and recs == want.records, (what, kept, want.kept, recs, want.records)
    assert out == want.out, what
    assert np.array_equal(starts, want.starts), what
    assert carry == want.carry, (what, carry, want.carry)


def test_reference_agrees_with_the_oracle_on_records_split_by_splitlines():
    """the reference pinned once: its stream cut at the separators gives the oracle the same sketch as the records a line-oriented
    parser reads (well-formed files only: bytes.splitlines also ends a line at a lone CR, which the parser does not)"""
    names = ["sweep-fasta-lf_header-p8191-crlf-lf", "sweep-fasta-crlf_pair-p8192-lf-nolf", "sweep-fasta-empty_line-p2047-lf-lf",
             "sweep-fasta-gt_midline-p16384-crlf-nolf", "sweep-fastq-line1-p8192-lf-lf", "sweep-fastq-line3-p16383-crlf-nolf",
             "long-header-8300-at8191", "fastq-quality-starts-with-@", "fasta-begins-on-sequence", "sweep-fastq-line0-p2048-crlf-lf"]
    for name in names:
        case = fc.by_name()[name]
        a, b = fc.records_of(case.raw, case.fastq), fc.records_by_splitlines(case.raw, case.fastq)
        assert len(a) == len(b), name
        for k in (5, 21):
            ma, mb = oracle.OracleMinHash(0, k, scaled=1, track_abundance=True), oracle.OracleMinHash(0, k, scaled=1, track_abundance=True)
            for r in a:
                ma.add_sequence(r, force=True)
            for r in b:
                mb.add_sequence(r, force=True)
            assert (k > 5 or len(ma.mins) > 0) and np.array_equal(ma.mins, mb.mins) and np.array_equal(ma.abunds, mb.abunds), (name, k)


def test_whole_files(emul):
    for case in fc.small_cases() + fc.big_cases():
        check(emul(case.raw, case.fastq), fc.expected(case.name), case.name)


@pytest.mark.parametrize("size", fc.PIECE_SIZES)
def test_pieces_with_the_carry_chained(emul, size):
    """every case of at most three blocks cut into pieces of `size` bytes and one empty piece: the whole file's answer.  Sizes from
    31 on cut every case all the way through; 1 and 7 do so for short cases and around the points of the others (fc.piece_cuts)"""
    for case in fc.piece_cases():
        check(emul(case.raw, case.fastq, cuts=fc.piece_cuts(case, size, full_from=31)), fc.expected(case.name), (case.name, size))


@pytest.mark.parametrize("cut", fc.BIG_CUTS)
def test_1025_blocks_in_two_pieces(emul, cut):
    "1,024 blocks first (one block per span), then 1,024 blocks and a byte (two per span, the last spans empty)"
    for case in fc.big_cases():
        cuts = [0, cut, cut, len(case.raw)]
        check(emul(case.raw, case.fastq, cuts=cuts), fc.expected(case.name), (case.name, cut))


def test_record_capacity(emul):
    "capacities 0, 1 and records - 1: nothing is written at or behind the capacity, the count still reports every record"
    cases = [c for c in fc.small_cases() + fc.big_cases() if fc.expected(c.name).records >= 2]
    assert len(cases) > 300
    for case in cases[::7] + list(fc.big_cases()):
        want = fc.expected(case.name)
        for cap in (0, 1, want.records - 1):
            out, starts, kept, recs, carry, guard = emul(case.raw, case.fastq, cap=cap, guard=4)
            assert (kept, recs, carry) == (want.kept, want.records, want.carry) and out == want.out, (case.name, cap)
            assert np.array_equal(starts, want.starts[:cap]), (case.name, cap)
            assert len(guard) == 4 and (guard == np.uint64(GUARD)).all(), (case.name, cap)


def _record(case, cuts, cap):
    want = fc.expected(case.name)
    n_starts = min(cap, want.records)
    pad = lambda b: b + bytes(-len(b) % 8)                                   # noqa: E731
    head = struct.pack("<6Q2B6x", len(case.raw), case.fastq, len(cuts), cap, want.kept, want.records, *want.carry)
    return head + pad(case.raw) + np.asarray(cuts, dtype=np.uint64).tobytes() + pad(want.out) + want.starts[:n_starts].tobytes()


def test_under_the_sanitizers(tmp_path):
    """the stand-alone program with -fsanitize=address,undefined over a case file written here: raw inputs and the reference's
    outputs.  Every case whole; the cases of at most three blocks in pieces, half of them at each size (every case at four
    sizes, fc.piece_cuts); the 1,025-block pair whole and each in two pieces at one of the two cuts; capacities 0, 1, records - 1.
    The program copies every piece into a buffer of its exact size, so a read in front of or behind a piece is a report."""
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){}",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime is not installed: " + probe.stderr.strip().splitlines()[-1])
    exe = build("fastx_emul_san", "-O2", "-g", "-DFASTX_EMUL_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover")
    path = tmp_path / "cases.bin"
    count = 0
    with open(path, "wb") as f:
        for case in fc.small_cases() + fc.big_cases():
            f.write(_record(case, [], len(case.raw) + 1))
            count += 1
        for i, size in enumerate(fc.PIECE_SIZES):
            for case in fc.piece_cases()[i % 2::2]:
                f.write(_record(case, fc.piece_cuts(case, size), len(case.raw) + 1))
                count += 1
        for case, cut in zip(fc.big_cases(), fc.BIG_CUTS):
            f.write(_record(case, [0, cut, cut, len(case.raw)], len(case.raw) + 1))
            count += 1
        for case in [c for c in fc.small_cases() if fc.expected(c.name).records >= 2][::7]:
            for cap in (0, 1, fc.expected(case.name).records - 1):
                f.write(_record(case, [], cap))
                count += 1
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == f"fastx ok: {count} cases", out.stderr[-4000:]
