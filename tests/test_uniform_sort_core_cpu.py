"""CPU check of the sort + unique for uniform keys (sourmash_amd/csrc/uniform_sort_core.hpp compiled for the host): the plan's rule and
the lane code of scatter rank, leaf sort and dedupe, walked with lanes as loop indices by tests/native/uniform_sort_emul.cpp against
std::sort + std::unique.  The program runs by itself -- nothing is loaded into this process -- plain and once more under
AddressSanitizer and UndefinedBehaviorSanitizer; it also takes the inputs of tests/test_gpu_uniform_sort.py (uniform_sort_cases.py)
and proves that the plan's own rule keeps every uniform one of them inside its leaves.  No GPU needed."""
import os
import re
import struct
import subprocess

import pytest

import uniform_sort_cases as uc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "uniform_sort_emul.cpp")
HDRS = [os.path.join(HERE, "..", "sourmash_amd", "csrc", "uniform_sort_core.hpp")]


def build(name, *flags):
    out = os.path.join(HERE, "native", name)
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(out) or os.path.getmtime(out) < newest:
        subprocess.check_call(["g++", "-std=c++17", "-Wall", *flags, "-o", out, SRC])
    return out


def sanitized():
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull], input="int main(){}",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("the sanitizer runtime is not installed: " + probe.stderr.strip().splitlines()[-1])
    return build("uniform_sort_emul_san", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover")


def run(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    last = out.stdout.strip().splitlines()[-1]
    m = re.fullmatch(r"uniform sort ok: (\d+) cases", last)
    assert m, out.stdout[-2000:]
    return int(m.group(1)), out.stdout


def test_builtin_cases():
    """the plan over sizes and thresholds (L = 255 / 256 / 257 / 258, thr = 2^64 - 1, thr = 20 / 40 / 2^24), and the whole
    pipeline on: sizes around the network's powers of two, leaf loads 0 / 1 / C - 1 / C / C + 1, keys on both sides of every
    leaf boundary, keys 0, 1, thr, thr + 1 and 2^64 - 1, counts below and above n_max, equal and alternating keys"""
    n, _ = run(build("uniform_sort_emul", "-O2"))
    assert n >= 300


def test_builtin_cases_under_the_sanitizers():
    n, _ = run(sanitized())
    assert n >= 300


def write_cases(path, cases):
    with open(path, "wb") as f:
        for c in cases:
            f.write(struct.pack("<5Q", len(c.keys), c.count, c.thr, c.want, len(c.keys)))
            f.write(c.keys.tobytes())


def test_the_gpu_tests_inputs(tmp_path):
    """every input of tests/test_gpu_uniform_sort.py through the emulation: right result, the form the GPU test expects, and
    the uniform ones stay inside their leaves by the plan's own rule (the program fails a case that must not fall back and does)"""
    cases = uc.cases()
    write_cases(tmp_path / "cases.bin", cases)
    n, text = run(build("uniform_sort_emul", "-O2"), str(tmp_path / "cases.bin"))
    assert n == len(cases)
    lines = [ln for ln in text.splitlines() if ln.startswith("case ")]
    assert len(lines) == len(cases)
    for c, ln in zip(cases, lines):
        m = re.fullmatch(r"case \d+: form (\d+) fellback (\d) distinct (\d+)", ln)
        assert m, ln
        assert int(m.group(1)) == c.form, (c.name, ln)
        assert int(m.group(2)) == c.want, (c.name, ln)
        if not c.want:
            assert int(m.group(3)) == len(uc.expected(c)[0]), (c.name, ln)


def test_the_gpu_tests_inputs_under_the_sanitizers(tmp_path):
    "the same file without its one large case, under the sanitizers"
    cases = [c for c in uc.cases() if len(c.keys) <= 200_000]
    write_cases(tmp_path / "cases.bin", cases)
    n, _ = run(sanitized(), str(tmp_path / "cases.bin"))
    assert n == len(cases)
