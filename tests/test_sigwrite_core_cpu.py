"""CPU check of the signature writer's rules (sourmash_amd/csrc/sigwrite_core.hpp compiled for the host) through an emulation of
sigwrite.hip with lanes as loop indices (tests/native/sigwrite_emul.cpp): decimal text, the per-lane MD5 against hashlib, the
literal code and its block header against zlib, the packer against zlib with guard words behind every output, and once more as a
stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer.  No GPU needed."""
import ctypes as C
import hashlib
import os
import subprocess
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "sigwrite_emul.cpp")
HDRS = [os.path.join(HERE, "..", "sourmash_amd", "csrc", "sigwrite_core.hpp")]
N_GUARD = 4
GUARD = 0xA5A5A5A5
MAX_CHUNK = 4096

EDGE_VALUES = sorted({1, 9, 10, 99, 2**64 - 1} | {10**k - 1 for k in range(1, 20)} | {10**k for k in range(1, 20)})


def build(name, *flags):
    out = os.path.join(HERE, "native", name)
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(out) or os.path.getmtime(out) < newest:
        subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", *flags, "-o", out, SRC])
    return out


@pytest.fixture(scope="module")
def emul():
    lib = C.CDLL(build("libsigwrite_emul.so", "-O2", "-shared", "-fPIC"))
    lib.sw_emul_decimal.argtypes = [C.c_uint64, C.c_void_p]
    lib.sw_emul_decimal.restype = C.c_uint32
    lib.sw_emul_md5.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.sw_emul_table.argtypes = [C.c_void_p]
    lib.sw_emul_header.argtypes = [C.c_void_p, C.c_uint32]
    lib.sw_emul_header.restype = C.c_uint32
    lib.sw_emul_deflate.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64]
    lib.sw_emul_deflate.restype = C.c_uint64
    return lib


def md5_rows(lib, ksize, rows):
    "digests of the rows through the emulated kernel (hex strings)"
    offsets = np.zeros(len(rows) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    hashes = np.array([np.uint64(h) for r in rows for h in r] + [np.uint64(0)], dtype=np.uint64)
    out = np.full(16 * len(rows) + N_GUARD, 0xA5, dtype=np.uint8)
    lib.sw_emul_md5(ksize, hashes.ctypes.data, offsets.ctypes.data, len(rows), out.ctypes.data)
    assert (out[16 * len(rows):] == 0xA5).all()
    return [out[16 * i:16 * i + 16].tobytes().hex() for i in range(len(rows))]


def want_md5(ksize, row):
    return hashlib.md5((str(ksize) + "".join(map(str, row))).encode()).hexdigest()


def rows_of_message_length(total, ksize=31):
    "a row of edge values whose message str(ksize) + digits has exactly `total` bytes"
    need = total - len(str(ksize))
    row = []
    while need >= 20:
        row.append(2**64 - 1)
        need -= 20
    if need:
        row.append(10**need - 1)
    assert len(str(ksize) + "".join(map(str, row))) == total
    return row


def deflate(lib, text, chunk, lanes=256):
    words = (len(text) * 15 + 2048) // 32 + 8
    out = np.full(words + N_GUARD, GUARD, dtype=np.uint32)
    n = lib.sw_emul_deflate(text, len(text), chunk, lanes, out.ctypes.data, words)
    assert n > 0
    assert (out[words:] == GUARD).all(), "guard words behind the output were written"
    return out[:words].tobytes()[:n]


def test_decimal_edges(emul):
    buf = np.zeros(20 + N_GUARD, dtype=np.uint8)
    for v in EDGE_VALUES:
        buf[:] = 0xA5
        nd = emul.sw_emul_decimal(v, buf.ctypes.data)
        assert nd == len(str(v)), v
        assert buf[:nd].tobytes().decode() == str(v), v
        assert (buf[nd:] == 0xA5).all(), v


def test_md5_block_edges(emul):
    "messages on every side of the 55 / 56 / 63 / 64 byte edges of the padding, one and two blocks up"
    rows = [rows_of_message_length(n) for n in (2, 3, 54, 55, 56, 57, 62, 63, 64, 65, 118, 119, 120, 121, 127, 128, 129, 183, 184, 1000)]
    rows[0] = []                                                     # the message is "31" alone
    got = md5_rows(emul, 31, rows)
    assert got == [want_md5(31, r) for r in rows]


def test_md5_lane_edges(emul):
    "63, 64 and 65 rows (a wave's lanes), rows of 0 .. 4 hashes and random rows of unlike lengths"
    rng = np.random.default_rng(3)
    for n in (63, 64, 65):
        rows = [[int(x) for x in rng.integers(0, 2**63, size=i % 7, dtype=np.uint64)] for i in range(n)]
        rows[-1] = [int(x) for x in rng.integers(0, 2**63, size=300, dtype=np.uint64)]
        assert md5_rows(emul, 21, rows) == [want_md5(21, r) for r in rows]
    rows = [EDGE_VALUES[:i] for i in range(5)] + [EDGE_VALUES]
    assert md5_rows(emul, 51, rows) == [want_md5(51, r) for r in rows]


def test_code_table(emul):
    table = np.zeros(257, dtype=np.uint32)
    emul.sw_emul_table(table.ctypes.data)
    lens = (table >> 16).astype(np.int64)
    assert len(lens) == 257 and lens.min() >= 1, "every symbol has a code"
    assert lens.max() <= 15
    assert sum(1 << (15 - int(l)) for l in lens) == 1 << 15, "Kraft sum is exactly 1"
    # a prefix code: no code is the beginning of another (codes are stored first bit in bit 0)
    codes = sorted("".join(str((int(t) >> b) & 1) for b in range(int(t) >> 16)) for t in table)
    assert all(not b.startswith(a) for a, b in zip(codes, codes[1:]))


def test_block_header_inflates_to_nothing(emul):
    "the host-built header followed by end-of-block is a whole deflate stream of no bytes"
    hdr = np.zeros(256, dtype=np.uint8)
    nbits = emul.sw_emul_header(hdr.ctypes.data, len(hdr))
    assert 0 < nbits <= 1274
    assert zlib.decompress(deflate(emul, b"", 64), wbits=-15) == b""
    assert deflate(emul, b"", 64)[:nbits // 8] == hdr[:nbits // 8].tobytes()


@pytest.mark.parametrize("chunk", [64, 1000, MAX_CHUNK])
def test_pack_round_trip(emul, chunk):
    rng = np.random.default_rng(chunk)
    for n in (0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 7):
        for text in (rng.integers(0, 256, size=n, dtype=np.uint8).tobytes(),
                     rng.choice(np.frombuffer(b"0123456789,", dtype=np.uint8), size=n).tobytes()):
            for lanes in (256, 1, 7):
                stream = deflate(emul, text, chunk, lanes)
                assert zlib.decompress(stream, wbits=-15) == text, (chunk, n, lanes)


def test_all_byte_values(emul):
    text = bytes(range(256)) * 3
    assert zlib.decompress(deflate(emul, text, 100), wbits=-15) == text


def test_standalone_under_sanitizers(tmp_path):
    exe = build("sigwrite_emul_san", "-O1", "-g", "-DSW_EMUL_MAIN", "-static-libasan", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
    rng = np.random.default_rng(11)
    cases, want = [], []
    for v in EDGE_VALUES:
        cases.append(f"dec {v}")
        want.append(str(v))
    for n in (2, 55, 56, 57, 63, 64, 65, 119, 120, 121, 500):
        row = rows_of_message_length(n) if n > 2 else []
        cases.append("md5 31 " + " ".join(map(str, row)))
        want.append(want_md5(31, row))
    texts = []
    for chunk in (64, MAX_CHUNK):
        for n in (0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 7):
            text = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
            cases.append(f"deflate {chunk} 256 {text.hex() or '-'}")
            texts.append(text)
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(cases) + "\n")
    res = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    assert lines[:len(want)] == want
    for line, text in zip(lines[len(want):], texts):
        assert zlib.decompress(bytes.fromhex(line), wbits=-15) == text
