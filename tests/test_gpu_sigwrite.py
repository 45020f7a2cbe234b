"""The signature writer on the GPU (csrc/sigwrite.hip, csrc/sigwrite.hpp): MD5 identities, signature JSON, literal-only gzip members
and the .sig / .sig.gz / .zip files of SketchSet.save / SketchSetWriter / sketch_file_to -- against hashlib, zlib, zipfile, the
library's own host serialiser (save_signatures_to_json) and its loader.  Run with -m gpu."""
import glob
import gzip
import hashlib
import json
import struct
import zipfile
import zlib

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

MAX_HASH_1000 = 18446744073709552                  # max_hash of scaled = 1000
EDGE_VALUES = sorted({1, 9, 10, 99, 2**64 - 1} | {10**k - 1 for k in range(1, 20)} | {10**k for k in range(1, 20)})
CHUNK = 4096                                        # the packer's chunk (csrc/sigwrite_core.hpp: SW_MAX_CHUNK)
NAMES = ['a "quoted" name', "back\\slash", "control\x01char\ttab", "Übergröße ß 基因组", "", "x" * 300]


@pytest.fixture(scope="module")
def sm():
    import torch  # noqa: F401
    import sourmash_amd
    assert sourmash_amd.gpu_available()
    return sourmash_amd


def md5_of(ksize, mins):
    return hashlib.md5((str(ksize) + "".join(map(str, mins))).encode()).hexdigest()


def sig_text(rows, *, ksize=31, max_hash=MAX_HASH_1000, num=0, names=None, filenames=None):
    "a .sig file of one flat DNA signature per row"
    docs = []
    for i, mins in enumerate(rows):
        d = {"class": "sourmash_signature", "email": "", "hash_function": "0.murmur64",
             "filename": filenames[i] if filenames else f"file{i}.fa"}
        name = names[i] if names else f"row {i}"
        if name is not None:
            d["name"] = name
        d.update({"license": "CC0", "signatures": [{"num": num, "ksize": ksize, "seed": 42, "max_hash": max_hash, "mins": [int(m) for m in mins],
                                                    "md5sum": md5_of(ksize, mins), "molecule": "DNA"}], "version": 0.4})
        docs.append(d)
    return json.dumps(docs, separators=(",", ":"), ensure_ascii=False).encode()


def load_rows(tmp_path, rows, tag="in", **kw):
    from sourmash_amd.index import SketchSet
    p = tmp_path / f"{tag}.sig"
    p.write_bytes(sig_text(rows, **kw))
    s = SketchSet.load(str(p))
    assert len(s) == len(rows)
    return s


def rand_rows(rng, sizes, top=MAX_HASH_1000):
    return [np.unique(rng.integers(1, top, size=n, dtype=np.uint64)).tolist() if n else [] for n in sizes]


def row_of_message_length(total, ksize=31):
    "ascending edge values whose message str(ksize) + digits has exactly `total` bytes"
    need = total - len(str(ksize))
    lens = []
    while need >= 20:
        lens.append(20)
        need -= 20
    if need:
        lens.append(need)
    # distinct ascending numbers: one of every length is not enough, so the 20-digit ones count down from 2^64 - 1
    row = sorted([10**n - 1 for n in lens if n < 20]) + sorted(2**64 - 1 - i for i in range(lens.count(20)))
    assert len(str(ksize) + "".join(map(str, row))) == total and len(set(row)) == len(row)
    return row


# ---- md5 ------------------------------------------------------------------------------------------------------------------------
def test_md5_small_rows_and_lane_edges(sm, tmp_path):
    from sourmash_amd.index import SketchSet
    rng = np.random.default_rng(1)
    for n in (5, 64, 65):
        rows = rand_rows(rng, [i % 5 for i in range(n)])
        s = load_rows(tmp_path, rows, tag=f"n{n}")
        want = [md5_of(31, r) for r in rows]
        assert s.md5sums() == want
        assert [s.minhash(r).md5sum() for r in range(0, n, 7)] == want[::7]
    # a set built from sketch handles
    mhs = []
    for r in rand_rows(rng, [0, 3, 70]):
        mh = sm.MinHash(0, 21, scaled=1000)
        mh.add_many(r)
        mhs.append(mh)
    assert SketchSet(mhs).md5sums() == [mh.md5sum() for mh in mhs]


def test_md5_block_edges(sm, tmp_path):
    "message lengths on every side of the 55 / 56 / 63 / 64 byte edges of the padding, in the first and second block"
    lengths = [54, 55, 56, 57, 62, 63, 64, 65, 118, 119, 120, 121, 127, 128, 129, 183, 184, 185]
    rows = [row_of_message_length(n) for n in lengths] + [EDGE_VALUES]
    s = load_rows(tmp_path, rows, max_hash=2**64 - 1)
    want = [md5_of(31, r) for r in rows]
    assert s.md5sums() == want
    assert [s.minhash(r).md5sum() for r in range(len(rows))] == want


def test_md5_raw_long_row_bound(sm):
    "one row just under and one just over a long-row bound of 4 blocks: the device and the host path give the same digests"
    import torch
    from sourmash_amd._lowlevel import lib
    from sourmash_amd.utils import rustcall
    rng = np.random.default_rng(2)
    bound = 4 * 64
    rows = [row_of_message_length(bound - 1), row_of_message_length(bound), row_of_message_length(bound + 1), row_of_message_length(bound + 700)]
    rows += rand_rows(rng, [0, 1, 12])
    offsets = np.zeros(len(rows) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    hashes = np.array([np.uint64(h) for r in rows for h in r], dtype=np.uint64)
    d_h = torch.from_numpy(hashes.view(np.int64)).cuda()
    d_o = torch.from_numpy(offsets).cuda()
    d_md5 = torch.full((16 * len(rows) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    on_host = rustcall(lib.smgpu_sigwrite_md5_raw, d_h.data_ptr(), d_o.data_ptr(), len(rows), 31, bound, d_md5.data_ptr(), None)
    assert on_host == 2                                              # bound + 1 and bound + 700; a message of exactly `bound` bytes stays
    got = d_md5.cpu().numpy()
    assert (got[16 * len(rows):] == 0xA5).all()
    assert [got[16 * i:16 * i + 16].tobytes().hex() for i in range(len(rows))] == [md5_of(31, r) for r in rows]
    # the library's own bound: everything on the device
    d_md5.fill_(0xA5)
    torch.cuda.synchronize()
    assert rustcall(lib.smgpu_sigwrite_md5_raw, d_h.data_ptr(), d_o.data_ptr(), len(rows), 31, 0, d_md5.data_ptr(), None) == 0
    got = d_md5.cpu().numpy()
    assert [got[16 * i:16 * i + 16].tobytes().hex() for i in range(len(rows))] == [md5_of(31, r) for r in rows]


def test_md5_of_reference_files(sm):
    "rows loaded from files the reference wrote: md5sums() is the file's own md5sum field"
    from sourmash_amd.index import SketchSet
    files = [golden("ecoli", "GCF_000005845.2_ASM584v2_genomic.fna.gz.sig"), golden("pairs", "47.fa.sig")]
    files += sorted(glob.glob(golden("gather", "GCF_*.sig")))
    for path in files:
        want = {}
        for sig in json.load(open(path)):
            for sk in sig["signatures"]:
                if sk["molecule"].lower() == "dna":
                    want.setdefault(sk["ksize"], []).append(sk["md5sum"])
        assert want
        for ksize, md5s in want.items():
            assert SketchSet.load(path, ksize=ksize, moltype="DNA").md5sums() == md5s, (path, ksize)


# ---- JSON -----------------------------------------------------------------------------------------------------------------------
def test_to_json_scaled_with_odd_names(sm, tmp_path):
    rng = np.random.default_rng(3)
    rows = rand_rows(rng, [0, 1, 2, 300, 5000, 64])
    s = load_rows(tmp_path, rows, names=NAMES, filenames=["f.fa", "", 'q"uote.fa', "ü.fa", "e.fa", "y" * 300])
    want = sm.save_signatures_to_json([s.signature(r) for r in range(len(s))])
    got = s.to_json()
    assert got == want
    assert [d.get("name", "") for d in json.loads(got)] == NAMES
    pick = [4, 0, 5, 0]
    assert s.to_json(rows=pick) == sm.save_signatures_to_json([s.signature(r) for r in pick])
    assert s.to_json(rows=[]) == b"[]"
    assert gzip.decompress(s.to_json(compression=1)) == want
    assert gzip.decompress(s.to_json(rows=pick, compression=5)) == s.to_json(rows=pick)


def test_to_json_num(sm, tmp_path):
    rng = np.random.default_rng(4)
    rows = rand_rows(rng, [500, 500, 17], top=2**64 - 1)
    s = load_rows(tmp_path, rows, ksize=21, max_hash=0, num=500)
    assert s.to_json() == sm.save_signatures_to_json([s.signature(r) for r in range(len(s))])


def test_array_and_zip_span_batches(sm, tmp_path, monkeypatch):
    "batches of a few rows: the array stays one document and one gzip member (the deflate stream carries on at the bit it ended)"
    from sourmash_amd.index import SketchSet
    rng = np.random.default_rng(12)
    rows = rand_rows(rng, [300, 0, 1, 299, 301, 5, 640, 0, 300, 300, 17, 300])
    s = load_rows(tmp_path, rows)
    want = sm.save_signatures_to_json([s.signature(r) for r in range(len(s))])
    monkeypatch.setenv("SMG_SIGWRITE_BATCH_BYTES", "16000")          # two rows of 300 hashes do not fit
    assert s.to_json() == want
    member = s.to_json(compression=1)
    assert zlib.decompress(member, wbits=31) == want
    assert struct.unpack("<II", member[-8:]) == (zlib.crc32(want), len(want))
    for name in ("b.sig", "b.sig.gz", "b.zip"):
        s.save(str(tmp_path / name))
    s.save(str(tmp_path / "stored.sig.gz"), compression=0)          # stored blocks, batch after batch
    assert (tmp_path / "b.sig").read_bytes() == want
    assert (tmp_path / "b.sig.gz").read_bytes() == member
    assert zlib.decompress((tmp_path / "stored.sig.gz").read_bytes(), wbits=31) == want
    assert s.md5sums() == [md5_of(31, r) for r in rows]
    monkeypatch.delenv("SMG_SIGWRITE_BATCH_BYTES")
    assert SketchSet.load(str(tmp_path / "b.zip")).to_json() == want


# ---- deflate --------------------------------------------------------------------------------------------------------------------
def deflate_raw(texts, compression, chunk):
    "-> the members smgpu_deflate_literals_raw makes of the documents"
    import torch
    from sourmash_amd._lowlevel import lib
    from sourmash_amd.utils import rustcall
    docs, blob = [], bytearray()
    for t in texts:
        blob += bytes(-len(blob) % 16)
        docs.append((len(blob), len(t)))
        blob += t
    blob += bytes(64)
    d_text = torch.from_numpy(np.frombuffer(bytes(blob), dtype=np.uint8).copy()).cuda()
    docs_a = np.array(docs, dtype=np.uint64).reshape(-1)
    members = np.zeros(2 * len(texts), dtype=np.uint64)
    cap = sum(len(t) * 2 + 512 for t in texts)
    guard = 64
    d_out = torch.full((cap + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = rustcall(lib.smgpu_deflate_literals_raw, d_text.data_ptr(), len(blob), docs_a.ctypes.data, len(texts), compression, chunk, d_out.data_ptr(), cap,
                 members.ctypes.data, None)
    assert 0 < n <= cap
    out = d_out.cpu().numpy()
    assert (out[n:] == 0xA5).all(), "bytes behind the output were written"
    out = out.tobytes()
    return [out[int(members[2 * i]):int(members[2 * i]) + int(members[2 * i + 1])] for i in range(len(texts))]


def check_members(members, texts):
    for m, t in zip(members, texts):
        assert m[:4] == b"\x1f\x8b\x08\x00" and m[4:8] == b"\0\0\0\0"
        assert zlib.decompress(m, wbits=31) == t
        assert struct.unpack("<II", m[-8:]) == (zlib.crc32(t), len(t) & 0xFFFFFFFF)


@pytest.mark.parametrize("chunk", [64, CHUNK])
def test_deflate_lengths_at_chunk_edges(sm, chunk):
    rng = np.random.default_rng(chunk)
    texts = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in (0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 7)]
    texts.append(bytes(range(256)) * 2)
    check_members(deflate_raw(texts, 1, chunk), texts)
    check_members(deflate_raw(texts, 0, chunk), texts)


@pytest.mark.parametrize("n_docs", [1, 64, 65])
def test_deflate_document_counts(sm, n_docs):
    rng = np.random.default_rng(n_docs)
    texts = [rng.integers(0, 256, size=int(rng.integers(0, 700)), dtype=np.uint8).tobytes() for _ in range(n_docs)]
    check_members(deflate_raw(texts, 1, 256), texts)


def test_stored_block_edge(sm):
    rng = np.random.default_rng(5)
    texts = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in (65535, 65536)]
    members = deflate_raw(texts, 0, 0)
    check_members(members, texts)
    assert [len(m) for m in members] == [18 + 5 + 65535, 18 + 2 * 5 + 65536]


@pytest.mark.parametrize("n_hashes", [1000, 5000])
def test_member_no_longer_than_zlib_level_1(sm, tmp_path, n_hashes):
    """Size condition: a row of uniform hashes below max_hash(1000) with a typical genome name packs into a member no longer than
    zlib level 1 of the same text plus the 18 bytes of gzip framing."""
    rng = np.random.default_rng(7)
    rows = rand_rows(rng, [n_hashes])
    s = load_rows(tmp_path, rows, names=["NC_000913.3 Escherichia coli str. K-12 substr. MG1655, complete genome"],
                  filenames=["GCF_000005845.2_ASM584v2_genomic.fna.gz"])
    text = s.to_json()
    member = deflate_raw([text], 1, 0)[0]
    check_members([member], [text])
    limit = len(zlib.compress(text, 1)) + 18
    print(f"sigwrite size: {n_hashes} hashes, text {len(text)}, member {len(member)}, zlib-1 + 18 = {limit}, ratio {len(member) / limit:.4f}")
    assert len(member) <= limit


# ---- zip ------------------------------------------------------------------------------------------------------------------------
def read_zip(path):
    with zipfile.ZipFile(path) as zf:
        assert zf.testzip() is None
        infos = zf.infolist()
        return infos, {i.filename: zf.read(i) for i in infos}


def test_zip_round_trip(sm, tmp_path):
    from sourmash_amd.index import SketchSet, _manifest_rows
    rng = np.random.default_rng(8)
    rows = rand_rows(rng, [0, 1, 40, 5000, 700, 3])
    fnames = ["f.fa", "", "g.fa", "h.fa", "i.fa", "j.fa"]
    s = load_rows(tmp_path, rows, names=NAMES, filenames=fnames)
    out = tmp_path / "out.zip"
    s.save(str(out))
    infos, data = read_zip(out)
    md5s = [md5_of(31, r) for r in rows]
    assert [i.filename for i in infos] == [f"signatures/{m}.sig.gz" for m in md5s] + ["SOURMASH-MANIFEST.csv"]
    assert all(i.external_attr >> 16 == 0o444 for i in infos)
    assert all(i.compress_type == zipfile.ZIP_STORED for i in infos[:-1]) and infos[-1].compress_type == zipfile.ZIP_DEFLATED
    assert all(i.date_time == (1980, 1, 1, 0, 0, 0) for i in infos)
    for r, m in enumerate(md5s):
        assert gzip.decompress(data[f"signatures/{m}.sig.gz"]) == s.to_json(rows=[r])
    man = _manifest_rows(data["SOURMASH-MANIFEST.csv"].decode("utf-8"))
    assert man == [dict(internal_location=f"signatures/{m}.sig.gz", md5=m, md5short=m[:8], ksize=31, moltype="DNA", num=0, scaled=1000,
                        n_hashes=len(rows[r]), with_abundance=False, name=NAMES[r], filename=fnames[r]) for r, m in enumerate(md5s)]
    back = SketchSet.load(str(out))
    assert list(back.sizes) == list(s.sizes) and back.to_json() == s.to_json()
    assert [(m["name"], m["filename"]) for m in back.manifest] == list(zip(NAMES, fnames))
    assert back.md5sums() == md5s
    # the same set again: the same bytes; compression 0: stored members, the same documents
    again = tmp_path / "again.zip"
    s.save(str(again))
    assert again.read_bytes() == out.read_bytes()
    stored = tmp_path / "stored.zip"
    s.save(str(stored), compression=0)
    assert SketchSet.load(str(stored)).to_json() == s.to_json()


def test_zip_duplicates(sm, tmp_path):
    from sourmash_amd.index import SketchSet, _manifest_rows
    rng = np.random.default_rng(9)
    same = rand_rows(rng, [50])[0]
    rows = [same, same, same, [], []]
    names = ["one", "one", "another", "short read 1", "short read 2"]
    fnames = ["f.fa"] * 5
    s = load_rows(tmp_path, rows, names=names, filenames=fnames)
    out = tmp_path / "dups.zip"
    s.save(str(out))
    infos, data = read_zip(out)
    m, e = md5_of(31, same), md5_of(31, [])
    assert [i.filename for i in infos] == [f"signatures/{m}.sig.gz", f"signatures/{m}.sig.gz_0", f"signatures/{e}.sig.gz", f"signatures/{e}.sig.gz_0",
                                           "SOURMASH-MANIFEST.csv"]
    man = _manifest_rows(data["SOURMASH-MANIFEST.csv"].decode("utf-8"))
    assert [r["internal_location"] for r in man] == [f"signatures/{m}.sig.gz", f"signatures/{m}.sig.gz", f"signatures/{m}.sig.gz_0",
                                                     f"signatures/{e}.sig.gz", f"signatures/{e}.sig.gz_0"]
    assert [r["name"] for r in man] == names
    assert json.loads(gzip.decompress(data[f"signatures/{m}.sig.gz_0"]))[0]["name"] == "another"
    assert json.loads(gzip.decompress(data[f"signatures/{e}.sig.gz_0"]))[0]["name"] == "short read 2"
    back = SketchSet.load(str(out))                                  # (the loader reads a member once, however many rows name it)
    assert {(r["name"], int(n)) for r, n in zip(back.manifest, back.sizes)} == set(zip(names, [50, 50, 50, 0, 0]))


def test_writer_takes_several_sets(sm, tmp_path):
    from sourmash_amd.index import SketchSet
    rng = np.random.default_rng(10)
    rows21, rows31 = rand_rows(rng, [30, 0, 7]), rand_rows(rng, [30, 0, 7])
    s21 = load_rows(tmp_path, rows21, tag="k21", ksize=21)
    s31 = load_rows(tmp_path, rows31, tag="k31", ksize=31)
    out = tmp_path / "two.zip"
    with sm.SketchSetWriter(str(out)) as w:
        w.add(s21)
        w.add(s31)
    infos, _ = read_zip(out)
    assert len(infos) == 7
    for k, s in ((21, s21), (31, s31)):
        back = SketchSet.load(str(out), ksize=k)
        assert back.to_json() == s.to_json()
    # names given by the caller stand in for the set's
    named = tmp_path / "named.sig"
    with sm.SketchSetWriter(str(named)) as w:
        w.add(s21, names=["a", "b", "c"], filenames=["x", "y", "z"])
    assert [(d["name"], d["filename"]) for d in json.loads(named.read_bytes())] == [("a", "x"), ("b", "y"), ("c", "z")]


def test_zip64(sm, tmp_path):
    "70,000 one-hash rows: more entries than a plain zip's 65,535"
    from sourmash_amd.index import SketchSet
    n = 70_000
    rows = [[i + 1] for i in range(n)]
    names = [f"r{i}" for i in range(n)]
    s = load_rows(tmp_path, rows, names=names, filenames=["reads.fq"] * n)
    out = tmp_path / "many.zip"
    s.save(str(out))
    with zipfile.ZipFile(out) as zf:
        listed = zf.namelist()
        assert len(listed) == n + 1 and listed[-1] == "SOURMASH-MANIFEST.csv"
        assert json.loads(gzip.decompress(zf.read(listed[n - 1])))[0]["signatures"][0]["mins"] == [n]
    back = SketchSet.load(str(out))
    assert len(back) == n and back.total_hashes == n
    assert [m["name"] for m in back.manifest] == names
    assert back.md5sums() == [md5_of(31, r) for r in rows]


def test_missing_directory_leaves_no_file(sm, tmp_path):
    s = load_rows(tmp_path, [[1, 2, 3]])
    for name in ("out.zip", "out.sig", "out.sig.gz"):
        target = tmp_path / "no_such_dir" / name
        with pytest.raises(Exception):
            s.save(str(target))
    assert not (tmp_path / "no_such_dir").exists()
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.sig"]


# ---- end to end ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    rng = np.random.default_rng(11)
    recs = [("chr1 first", 4000), ("tiny", 12), ("chr2", 2500), ("tiny too", 5), ("chr3 last", 3100)]
    p = tmp_path_factory.mktemp("fa") / "genome.fa"
    with open(p, "w") as fh:
        for name, n in recs:
            seq = "".join(rng.choice(list("ACGT"), size=n))
            fh.write(f">{name}\n" + "\n".join(seq[i:i + 70] for i in range(0, n, 70)) + "\n")
    return str(p)


def sig_keys(sigs):
    "what identifies the sketches of these signatures, one entry per sketch (sketch_file puts a record's ksizes into one signature)"
    return sorted((mh.ksize, sig.name, sig.filename, mh.md5sum(), tuple(sorted(mh.hashes))) for sig in sigs for mh in sig.minhashes())


def test_sketch_file_to_zip(sm, tmp_path, fasta):
    from sourmash_amd.index import SketchSet
    from sourmash_amd.sketch import sketch_file, sketch_file_to
    params = "k=21,k=31,scaled=100"
    want = sketch_file(fasta, params, singleton=True)
    out = tmp_path / "reads.zip"
    assert len(want) == 5 and len(sig_keys(want)) == 10
    assert sketch_file_to(fasta, str(out), params, singleton=True) == 10
    for k in (21, 31):
        back = SketchSet.load(str(out), ksize=k)
        assert sig_keys(back.signature(r) for r in range(len(back))) == [key for key in sig_keys(want) if key[0] == k]
        assert back.md5sums() == [m["md5"] for m in back.manifest]
    # the two records shorter than k give empty sketches of different names: one member and one _0 per ksize
    with zipfile.ZipFile(out) as zf:
        assert sum(n.endswith(".sig.gz_0") for n in zf.namelist()) == 2 and len(zf.namelist()) == 11


@pytest.mark.parametrize("suffix", [".sig", ".sig.gz"])
def test_sketch_file_to_sig(sm, tmp_path, fasta, suffix):
    from sourmash_amd.sketch import sketch_file, sketch_file_to
    params = "k=21,k=31,scaled=100"
    want = sketch_file(fasta, params, singleton=True)
    out = tmp_path / ("reads" + suffix)
    sketch_file_to(fasta, str(out), params, singleton=True)
    raw = out.read_bytes()
    assert (raw[:2] == b"\x1f\x8b") == (suffix == ".sig.gz")
    if suffix == ".sig.gz":
        assert zlib.decompress(raw, wbits=31) == gzip.decompress(raw)          # one member
    got = list(sm.load_signatures_from_json(raw))
    assert len(got) == 10 and sig_keys(got) == sig_keys(want)


# ---- sets from device tensors, sets named afterwards -------------------------------------------------------------------------------
def test_from_csr(sm):
    "rows of a CSR held in tensors: an offsets base other than 0, names and file names, a num set, a protein ksize"
    import torch
    from sourmash_amd.index import SketchSet
    rng = np.random.default_rng(13)
    rows = rand_rows(rng, [3, 0, 40, 500], top=2**63)
    front = [7, 8, 9, 10, 11]                                        # hashes in front of the first row: offsets[0] = 5
    hashes = torch.tensor(front + [h for r in rows for h in r], dtype=torch.int64).cuda()
    offsets = torch.tensor(np.cumsum([len(front)] + [len(r) for r in rows]), dtype=torch.int64).cuda()
    names, fnames = ["a", "", 'q"', "ü"], ["f.fa", "g.fa", "", "h.fa"]
    for kw, json_k, molecule in ((dict(ksize=21, num=500), 21, "DNA"), (dict(ksize=10, scaled=200, moltype="protein"), 30, "protein")):
        s = SketchSet.from_csr(hashes, offsets, names=names, filenames=fnames, **kw)
        assert len(s) == 4 and list(s.sizes) == [len(r) for r in rows]
        assert [(m["name"], m["filename"], m["ksize"], m["moltype"]) for m in s.manifest] == [(n, f, kw["ksize"], molecule) for n, f in zip(names, fnames)]
        assert s.md5sums() == [md5_of(json_k, r) for r in rows]
        assert [sorted(s.minhash(r).hashes) for r in range(4)] == rows
        docs = json.loads(s.to_json())
        assert s.to_json() == sm.save_signatures_to_json([s.signature(r) for r in range(4)])
        assert [d["signatures"][0]["ksize"] for d in docs] == [json_k] * 4 and docs[0]["signatures"][0]["num"] == kw.get("num", 0)
        assert [d["signatures"][0]["mins"] for d in docs] == rows
    with pytest.raises(Exception, match="ascend"):
        SketchSet.from_csr(hashes, torch.tensor([5, 3, 9], dtype=torch.int64).cuda(), ksize=21, scaled=1000)


def test_record_by_record_set_is_written_with_its_names(sm, tmp_path, fasta):
    "SketchSet.sketch_file beyond the one-pass path (k = 89): to_json and save write the names its manifest shows"
    from sourmash_amd.index import SketchSet
    s = SketchSet.sketch_file(fasta, ksize=89, scaled=100)
    names = [m["name"] for m in s.manifest]
    assert names == ["chr1 first", "tiny", "chr2", "tiny too", "chr3 last"]
    docs = json.loads(s.to_json())
    assert [d.get("name", "") for d in docs] == names and all(d["filename"] == fasta for d in docs)
    s.save(str(tmp_path / "k89.zip"))
    back = SketchSet.load(str(tmp_path / "k89.zip"))
    assert sorted(m["name"] for m in back.manifest) == sorted(names) and back.total_hashes == s.total_hashes
    # a set of sketch handles, named afterwards
    mh = sm.MinHash(0, 21, scaled=1000)
    mh.add_many([5, 6, 7])
    t = SketchSet([mh])
    assert "name" not in json.loads(t.to_json())[0]
    t.set_names(["given"], ["g.fa"])
    assert [(d["name"], d["filename"]) for d in json.loads(t.to_json())] == [("given", "g.fa")]
    # abundance sketches are not for this writer
    ab = sm.MinHash(0, 21, scaled=1000, track_abundance=True)
    ab.add_many([5, 6, 7])
    with pytest.raises(Exception, match="abundance"):
        SketchSet([ab]).to_json()


@pytest.mark.parametrize("params,singleton,n_sigs", [("k=21,k=31,num=50", True, 5), ("k=21,k=31,scaled=100", False, 1)])
def test_sketch_file_to_beyond_the_records_path(sm, tmp_path, fasta, params, singleton, n_sigs):
    "num sketches / one signature per file: sketch_file's signatures, every ksize of them, into .zip and .sig"
    from sourmash_amd.index import SketchSet
    from sourmash_amd.sketch import sketch_file, sketch_file_to
    want = sketch_file(fasta, params, singleton=singleton)
    assert len(want) == n_sigs and len(sig_keys(want)) == 2 * n_sigs
    for name in ("o.zip", "o.sig", "o.sig.gz"):
        assert sketch_file_to(fasta, str(tmp_path / name), params, singleton=singleton) == 2 * n_sigs
    for name in ("o.sig", "o.sig.gz"):
        assert sig_keys(sm.load_signatures_from_json((tmp_path / name).read_bytes())) == sig_keys(want)
    got = []
    for k in (21, 31):
        back = SketchSet.load(str(tmp_path / "o.zip"), ksize=k)
        assert len(back) >= 1
        got += sig_keys(back.signature(r) for r in range(len(back)))
    # (the loader reads a member once: the empty sketches of the two short records share md5, and name apart, a member each)
    assert sorted(got) == sig_keys(want)


def test_raw_deflate_wants_an_aligned_text(sm):
    import torch
    from sourmash_amd._lowlevel import lib
    from sourmash_amd.utils import rustcall
    d_text = torch.zeros(256, dtype=torch.uint8, device="cuda")
    docs = np.array([0, 32], dtype=np.uint64)
    members = np.zeros(2, dtype=np.uint64)
    d_out = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(Exception, match="aligned"):
        rustcall(lib.smgpu_deflate_literals_raw, d_text.data_ptr() + 4, 64, docs.ctypes.data, 1, 1, 0, d_out.data_ptr(), 1024, members.ctypes.data, None)
