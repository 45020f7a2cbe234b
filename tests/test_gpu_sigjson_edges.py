"""GPU parity of the signature JSON array parser (sourmash_amd/csrc/sigjson.hip) at every seam of its two kernels -- ballot tile,
lane, chunk, look-ahead, the 16-byte line a chunk is loaded from, 2^64, keep_max -- through smgpu_sigjson_parse_raw: the named
and random cases of tests/sigjson_cases.py in a handful of text blocks, one call and one read-back per block, checked against
the reference written from the rules (contract (a), (b), (c) of sigjson_cases) and bit for bit against the host emulation of the
kernels.  Then named documents as whole signatures through SketchSet.load, with the path that parsed them asserted.
Run with -m gpu."""
import gzip
import json

import numpy as np
import pytest

import sigjson_cases as sc
from test_gpu_sigload import counters, md5_of, same_collection, write_zip
from test_sigjson_core_cpu import load_emul

pytestmark = pytest.mark.gpu

N_GUARD = 4
BEHIND = b",9,]7"                                # what stands in the padding behind a text block: nothing of it may be parsed


@pytest.fixture(scope="module")
def sm():
    import torch  # noqa: F401
    import sourmash_amd
    import sourmash_amd.device  # noqa: F401
    assert sourmash_amd.gpu_available(), "these tests need a real GPU"
    return sourmash_amd


@pytest.fixture(scope="module")
def emul():
    return load_emul()


def run_block(sm, block, n_values, base=0):
    """one call of the raw entry on a block whose first byte has the address `base` modulo 16 (device allocations begin on a
    line), one read-back of the values with their guard words -> what check_block takes"""
    import torch
    from sourmash_amd.device import sigjson_parse, sigjson_text_pad
    pad = sigjson_text_pad()
    assert pad == sc.TEXT_PAD
    h = np.frombuffer(bytes(base) + block.text + (BEHIND * pad)[:pad], dtype=np.uint8)
    d_text = torch.from_numpy(h.copy()).cuda()[base:]
    assert d_text.data_ptr() % 16 == base
    d_values = torch.from_numpy(np.full(n_values + N_GUARD, sc.GUARD, dtype=np.uint64).view(np.int64)).cuda()
    spans = np.full(len(block.docs) * sc.MAX_SPANS * sc.SPAN.itemsize, 0xA5, dtype=np.uint8).view(sc.SPAN)
    spans, flags, parsed, got_values = sigjson_parse(d_text, len(block.text), block.docs, block.keep_max, d_values, spans=spans)
    values = d_values.cpu().numpy().view(np.uint64)
    assert (values[n_values:] == np.uint64(sc.GUARD)).all(), block.name                          # (guard words behind the value block)
    jobs, where, planned_values = sc.plan(block.docs, spans, flags)
    assert planned_values == got_values == n_values and len(parsed) == len(jobs), (block.name, planned_values, got_values, n_values)
    return spans, flags, jobs, where, values[:n_values], parsed


def test_every_block_against_the_reference_and_the_emulation(sm, emul):
    taken = set()
    for block in sc.blocks():
        want = emul(block, 0)
        got = run_block(sm, block, len(want[4]))
        taken.update(sc.check_block(block, *got, ("device", block.name)))
        for g, w, what in zip(got, want, ("spans", "flags", "jobs", "where", "values", "parsed")):
            assert (g == w) if what == "where" else (g.tobytes() == w.tobytes()), (block.name, what)
    must = {c.name for c in sc.all_cases() if sc.takeable(c.name)}
    assert must <= taken and len(must) > 500, sorted(must - taken)[:10]


@pytest.mark.parametrize("base", [5, 15])
def test_blocks_that_do_not_begin_on_a_line(sm, emul, base):
    "the text pointer itself off a 16-byte line: every shift moves, the first chunk's line begins in front of the text"
    for block in [b for b in sc.blocks() if len(b.text) < 100_000]:
        want = emul(block, base)
        got = run_block(sm, block, len(want[4]), base=base)
        sc.check_block(block, *got, ("device", block.name, base))
        assert got[4].tobytes() == want[4].tobytes() and got[5].tobytes() == want[5].tobytes(), (block.name, base)


def test_refusals(sm):
    import torch
    from sourmash_amd._lowlevel import lib
    from sourmash_amd.device import sigjson_parse
    from sourmash_amd.utils import rustcall
    text = torch.zeros(64, dtype=torch.uint8, device="cuda")
    values = torch.zeros(8, dtype=torch.int64, device="cuda")
    with pytest.raises(Exception, match="outside the text"):
        sigjson_parse(text, 40, [(30, 11)], 0, values)
    with pytest.raises(Exception, match="outside the text"):
        sigjson_parse(text, 40, [(41, 0)], 0, values)
    host = np.zeros(64, dtype=np.uint64)
    args = [text.data_ptr(), 40, host.ctypes.data, 1, 0, host.ctypes.data, host.ctypes.data, values.data_ptr(), 8, host.ctypes.data, 8, host.ctypes.data, None]
    for null in (0, 2, 5, 6, 7, 9, 11):
        a = list(args)
        a[null] = None
        with pytest.raises(Exception, match="null pointer"):
            rustcall(lib.smgpu_sigjson_parse_raw, *a)
    h = np.frombuffer(b'{"mins":[1,2,3]}' + bytes(48), dtype=np.uint8).copy()
    with pytest.raises(Exception, match="do not fit"):
        sigjson_parse(torch.from_numpy(h).cuda(), 16, [(0, 16)], 0, values[:2])


# ---- whole signatures through the loader ------------------------------------------------------------------------------------------
MAX_HASH_1000 = 18446744073709551


def signature(names, num=0, max_hash=0, indent=None, name="a name"):
    "a signature document with one ksize-31 sketch per named case, its `mins` array the case's bytes as they are"
    sketches = []
    for i, n in enumerate(names):
        values = sc.ref_array(sc.array_body(n), sc.U64)[1]
        sketches.append({"num": num, "ksize": 31, "seed": 42, "max_hash": max_hash, "mins": [f"@@{i}@@"], "md5sum": md5_of(31, [v & sc.U64 for v in values]),
                         "molecule": "dna"})
    doc = [{"class": "sourmash_signature", "email": "", "hash_function": "0.murmur64", "filename": "f.fa", "name": name, "license": "CC0",
            "signatures": sketches, "version": 0.4}]
    text = json.dumps(doc, indent=indent, separators=None if indent else (",", ":")).encode()
    for i, n in enumerate(names):
        a, b = text.index(b'"@@%d@@"' % i), text.index(b'"@@%d@@"' % i) + len(b'"@@%d@@"' % i)
        a, b = text.rindex(b"[", 0, a) + 1, text.index(b"]", b)
        text = text[:a] + sc.array_body(n) + text[b:]
    return text


NUM_DOCS = {            # `num` sketches (no max_hash): values up to 2^64 - 1
    "sweep-4096-20": ["sweep-comma-at-4096-20-d20"], "sweep-4096+0": ["sweep-comma-at-4096+0-d19"], "sweep-8192-1": ["sweep-comma-at-8192-1-d20"],
    "sweep-4032+1": ["sweep-comma-at-4032+1-d20"], "sweep-64-22": ["sweep-comma-at-64-22-d19"], "u64-max": ["limit-u64-max-last"],
    "u64-max-across-4096": ["limit-u64-max-across-byte-4096"], "three-chunks": ["size-12289-bytes"], "stretch-63": ["last-digit-at-4158-behind-comma-at-4095"],
    "8-arrays": ["size-63-bytes", "size-64-bytes", "size-65-bytes", "size-4095-bytes", "size-4096-bytes", "size-4097-bytes", "size-4160-bytes",
                 "order-single-value"],
}
SCALED_DOCS = {         # scaled = 1000 sketches loaded with scaled = 2000: the kept prefix is counted against keep_max = sigjson_cases.KM
    "keep-max-last": ["order-keep-max-exactly-last"], "keep-max-middle": ["order-keep-max-exactly-in-the-middle-all-below-twice-keep-max"],
    "indent-2": ["sep-indent-2-form-300-values-around-keep-max"],
}
HOST_DOCS = {           # what the parser must hand to the host loader
    "2^64": ["limit-2^64-last"], "equal-pair-across-a-chunk": ["order-equal-pair-at-across-a-chunk"],
    "white-space-run-65-at-the-chunk's-last-comma": ["sep-white-space-run-65-behind-comma-chunk-last-comma"],
    "9-arrays": ["size-63-bytes", "size-64-bytes", "size-65-bytes", "size-4095-bytes", "size-4096-bytes", "size-4097-bytes", "size-4160-bytes",
                 "order-single-value", "order-ascending-300-values"],
}


def _load_each_and_zipped(sm, tmp_path, docs, label, on_device, **sel):
    "every document gzipped on its own, then all of them in one zip: device == host loader, and the counters say who parsed"
    paths = []
    for k, (name, doc) in enumerate(docs.items()):
        p = tmp_path / f"{label}{k}.sig.gz"
        p.write_bytes(gzip.compress(doc))
        before = counters()
        dev, _ = same_collection(sm, str(p), **sel)
        after = counters()
        assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if on_device else (0, 1)), (name, before, after)
        assert len(dev) == doc.count(b'"ksize"'), name
        paths.append(str(p))
    z = str(tmp_path / f"{label}.zip")
    write_zip(z, [(doc, []) for doc in docs.values()], manifest_rows=False)
    before = counters()
    dev, _ = same_collection(sm, z, **sel)
    after = counters()
    assert (after[0] - before[0], after[1] - before[1]) == ((len(docs), 0) if on_device else (0, len(docs))), (label, before, after)
    return dev


def test_named_documents_load_on_the_device_path(sm, tmp_path):
    for names in list(NUM_DOCS.values()) + list(SCALED_DOCS.values()):
        assert all(sc.takeable(n) for n in names), names                                         # the reference's word, not the parser's
    num = {k: signature(v, num=100000, name=k) for k, v in NUM_DOCS.items()}
    dev = _load_each_and_zipped(sm, tmp_path, num, "num", True, ksize=31, moltype="DNA")
    assert len(dev) == sum(len(v) for v in NUM_DOCS.values())
    row = list(NUM_DOCS).index("u64-max")
    assert max(dev.minhash(row).hashes) == sc.U64
    scaled = {k: signature(v, max_hash=MAX_HASH_1000, indent=2 if k == "indent-2" else None, name=k) for k, v in SCALED_DOCS.items()}
    _load_each_and_zipped(sm, tmp_path, scaled, "scaled", True, ksize=31, moltype="DNA")
    dev = _load_each_and_zipped(sm, tmp_path, scaled, "down", True, ksize=31, moltype="DNA", scaled=2000)
    want = [sc.expected(v[0]).arrays[0].n_kept for v in SCALED_DOCS.values()]                    # keep_max itself is kept, keep_max + 1 is not
    assert list(dev.sizes) == want and want == [3, 3, 151], (list(dev.sizes), want)


def test_flagged_documents_go_to_the_host_and_come_out_as_its(sm, tmp_path):
    for k, names in HOST_DOCS.items():
        assert len(names) > sc.MAX_SPANS or not sc.takeable(names[0]), k                            # the reference's word, not the parser's
    docs = {k: signature(v, num=100000, name=k) for k, v in HOST_DOCS.items()}
    _load_each_and_zipped(sm, tmp_path, docs, "host", False, ksize=31, moltype="DNA")
