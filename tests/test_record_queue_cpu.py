"""The deferred-record queue's shared rule (csrc/record_queue.hpp: valid prefix, append, release), compiled alone for the host
and checked by tests/native/record_queue_check.cpp against a restatement of the reference's streaming walk.  No GPU, no HIP."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "record_queue_check.cpp")


def test_record_queue_rule(tmp_path):
    exe = str(tmp_path / "record_queue_check")
    flags = ["-O1", "-g", "-std=c++17", "-Wall", "-Werror"]
    # a stand-alone program: under AddressSanitizer + UBSan where gcc's runtime is installed, plain otherwise
    if os.path.isabs(subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()):
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover"]
    subprocess.check_call(["g++", *flags, "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-4000:]
    m = re.fullmatch(r"record queue ok: (\d+) cases", out.stdout.strip().splitlines()[-1])
    assert m, out.stdout[-2000:]
    # 6 ksizes x 5 lengths x (no bad byte + every position x 5 byte values, most of them twice) x force x pre-scanned
    assert int(m.group(1)) > 10000
