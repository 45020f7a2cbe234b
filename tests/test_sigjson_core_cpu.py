"""CPU check of the signature JSON array parser's rules (sourmash_amd/csrc/sigjson_core.hpp compiled for the host) through an
emulation of sigjson.hip's two kernels with lanes as loop indices (tests/native/sigjson_emul.cpp), against the reference and the
cases of tests/sigjson_cases.py: every text block at several addresses modulo 16, guard words behind every output, and once
more as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer.  No GPU needed."""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import sigjson_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "sigjson_emul.cpp")
HDRS = [os.path.join(HERE, "..", "sourmash_amd", "csrc", "sigjson_core.hpp")]
N_GUARD = 4


def build(name, *flags):
    out = os.path.join(HERE, "native", name)
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(out) or os.path.getmtime(out) < newest:
        subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", *flags, "-o", out, SRC])
    return out


def load_emul():
    """-> run(block, base_mod16) -> (spans, flags, jobs, where, values, parsed): the emulation on a text block whose first byte has
    the address base_mod16 modulo 16.  Spans and values begin as guard bytes and have N_GUARD guard entries behind them, which are
    checked here; the jobs are planned from the emulation's own span records (sigjson_cases.plan)."""
    lib = C.CDLL(build("libsigjson_emul.so", "-O2", "-shared", "-fPIC"))
    lib.sigjson_emul_spans.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.sigjson_emul_parse.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64]
    guard8 = np.uint8(0xA5)

    def run(block, base_mod16=0):
        n = len(block.docs)
        docs = np.array(block.docs, dtype=np.uint64).reshape(-1, 2)
        spans = np.full((n * sc.MAX_SPANS + N_GUARD) * sc.SPAN.itemsize, guard8, dtype=np.uint8)
        flags = np.full(n + N_GUARD, 0xA5A5A5A5, dtype=np.uint32)
        lib.sigjson_emul_spans(block.text, len(block.text), docs.ctypes.data, n, spans.ctypes.data, flags.ctypes.data)
        assert (spans[n * sc.MAX_SPANS * sc.SPAN.itemsize:] == guard8).all() and (flags[n:] == 0xA5A5A5A5).all(), block.name
        spans = spans[:n * sc.MAX_SPANS * sc.SPAN.itemsize].view(sc.SPAN)
        flags = flags[:n]
        jobs, where, n_values = sc.plan(block.docs, spans, flags)
        values = np.full(n_values + N_GUARD, sc.GUARD, dtype=np.uint64)
        parsed = np.full((len(jobs) + N_GUARD) * sc.PARSED.itemsize, guard8, dtype=np.uint8)
        lib.sigjson_emul_parse(block.text, len(block.text), base_mod16, jobs.ctypes.data, len(jobs), values.ctypes.data, parsed.ctypes.data, block.keep_max)
        assert (values[n_values:] == np.uint64(sc.GUARD)).all() and (parsed[len(jobs) * sc.PARSED.itemsize:] == guard8).all(), block.name
        return spans, flags, jobs, where, values[:n_values], parsed[:len(jobs) * sc.PARSED.itemsize].view(sc.PARSED)
    return run


@pytest.fixture(scope="module")
def emul():
    return load_emul()


def _mins_of(obj, out):
    "the `mins` lists of a parsed JSON document, in document order"
    if isinstance(obj, dict):
        for k, v in obj.items():
            if k == "mins" and isinstance(v, list):
                out.append(v)
            else:
                _mins_of(v, out)
    elif isinstance(obj, list):
        for v in obj:
            _mins_of(v, out)
    return out


def test_reference_agrees_with_json_loads():
    """the reference pinned once, independently: for every case it calls un-odd and plain, json.loads of the whole document gives the
    same integers.  (A fragment cut behind its array gets its closing brace first.)  Leading zeros are the one thing the
    reference -- like the host loader and the parser -- takes and JSON does not: those documents must fail json.loads."""
    checked = zeros = 0
    for case in sc.all_cases():
        exp = sc.expected(case.name)
        if exp.doc_odd or any(s.odd for s in exp.spans) or not all(a.plain for a in exp.arrays):
            continue
        doc = case.doc + case.json_fix
        if any(re.search(rb"(?<![0-9])0[0-9]", case.doc[s.begin:s.end]) for s in exp.spans):
            with pytest.raises(json.JSONDecodeError):
                json.loads(doc)
            zeros += 1
            continue
        got = _mins_of(json.loads(doc), [])
        assert got == [a.values for a in exp.arrays], case.name
        assert all(isinstance(v, int) for a in got for v in a), case.name
        checked += 1
    assert checked > 500 and zeros >= 6, (checked, zeros)


def test_may_fall_back_is_what_the_63_byte_rule_says():
    "the tag is on exactly the cases the reference computes from the rule, and on less than a tenth of the random ones"
    tagged = {c.name for c in sc.all_cases() if c.may_fall_back}
    assert tagged == {c.name for c in sc.all_cases() if sc.computed_may_fall_back(c.name)}
    n_random = sum(c.may_fall_back for c in sc.random_cases())
    assert 0 < n_random < len(sc.random_cases()) / 10, n_random
    assert len(sc.random_cases()) == 300 and sum("-" in c.name[len("random-000"):] for c in sc.random_cases()) >= 60


@pytest.mark.parametrize("base_mod16", [0, 1, 8, 15])
def test_every_block_against_the_reference(emul, base_mod16):
    """contract (a), (b), (c) on every case, the blocks at four addresses modulo 16 (the documents' own offsets cover all 16 for
    the alignment cases); every takeable case is taken"""
    taken = set()
    for block in sc.blocks():
        got = emul(block, base_mod16)
        taken.update(sc.check_block(block, *got, ("emulation", block.name, base_mod16)))
    must = {c.name for c in sc.all_cases() if sc.takeable(c.name)}
    assert must <= taken and len(must) > 500, sorted(must - taken)[:10]


def test_all_16_shifts_are_met():
    "the address of an array's first byte modulo 16, over the named cases with one array at least, as the blocks lay them out"
    seen = set()
    for block in sc.blocks():
        for (off, _), case in zip(block.docs, block.cases):
            spans = sc.expected(case.name).spans
            if spans and case.name.startswith("align-"):
                assert (off + spans[0].begin) % 16 == case.align, case.name
                seen.add(((off + spans[0].begin) % 16, case.name.split("-", 2)[2]))
    assert len(seen) == 16 * 5


def _record(block, base_mod16, got):
    spans, flags, jobs, _, values, parsed = got
    pad = lambda b: b + bytes(-len(b) % 8)                                   # noqa: E731
    head = struct.pack("<6Q", len(block.text), len(block.docs), base_mod16, block.keep_max, len(jobs), len(values))
    docs = np.array(block.docs, dtype=np.uint64).tobytes()
    return head + pad(block.text) + docs + spans.tobytes() + pad(flags.tobytes()) + jobs.tobytes() + values.tobytes() + parsed.tobytes()


def test_under_the_sanitizers(emul, tmp_path):
    """the stand-alone program with -fsanitize=address,undefined over a case file written here: every block at base addresses 0, 5
    and 15 modulo 16, with the outputs the emulation gave above (checked against the reference there).  The program holds every
    document, the text block with its padding, the chunk buffer and the value array in allocations of their exact sizes, so a
    read or write outside any of them is a report."""
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){}",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime is not installed: " + probe.stderr.strip().splitlines()[-1])
    exe = build("sigjson_emul_san", "-O1", "-g", "-DSIGJSON_EMUL_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover")
    path = tmp_path / "cases.bin"
    count = 0
    with open(path, "wb") as f:
        for base in (0, 5, 15):
            for block in sc.blocks():
                f.write(_record(block, base, emul(block, base)))
                count += 1
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == f"sigjson ok: {count} cases", out.stderr[-4000:]
