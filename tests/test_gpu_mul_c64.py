"""The hash built on the limb-wise 64-bit constant multiply (csrc/murmur3.hpp, mul_c64), on the GPU: one seeded buffer sketched at
k = 21, 31, 51, 88, 89 and 128 -- the appending and the per-position form of the register-window kernel, limb form (21, 31, 88)
and plain form (51) among them, and the run-time-k kernel past 88 -- and through the protein and HyperLogLog entry points, all
against the oracle.  The parity suites cover the same paths case by case; this one keeps the multiply's reach in one place.
Run with -m gpu."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

KS = [21, 31, 51, 88, 89, 128]


@pytest.fixture(scope="module")
def sm():
    import torch  # noqa: F401
    import sourmash_amd
    assert sourmash_amd.gpu_available(), "these tests need a real GPU"
    return sourmash_amd


@pytest.fixture(scope="module")
def buf():
    rng = np.random.default_rng(20240531)
    s = bytearray(rng.choice(np.frombuffer(b"ACGTacgt", dtype=np.uint8), size=400_003).tobytes())
    for i in range(13, len(s), 4099):
        s[i] = ord("N")
    return bytes(s)


@pytest.mark.parametrize("k", KS)
def test_dna_sketch_equals_oracle(sm, buf, k):
    for scaled in (1000, 7):
        mh = sm.MinHash(0, k, scaled=scaled)
        mh.add_sequence_buffer(buf)
        want = oracle.sketch_dna_bulk(buf, k, scaled=scaled, nthreads=4)
        assert len(want) > 0
        assert np.array_equal(mh._mins_array(), want), (k, scaled)
    head = buf[:9000]
    ordered = sm.MinHash(0, k, scaled=1).seq_to_hashes(head.decode(), force=True, bad_kmers_as_zeroes=True)
    assert ordered == [h or 0 for h in oracle.seq_to_hashes(head, k, force=True, bad_kmers_as_zeroes=True)], k


def test_multi_ksize_pass_equals_oracle(sm, buf, tmp_path):
    "k = 21, 31 and 51 of one file: the one-pass kernel of sketch_multi.hip (its largest ksize keeps the plain multiply)"
    from sourmash_amd.sketch import sketch_file
    path = str(tmp_path / "one.fa")
    with open(path, "wb") as f:
        f.write(b">one\n" + b"\n".join(buf[i:i + 70] for i in range(0, len(buf), 70)) + b"\n")
    sig, = sketch_file(path, "k=21,k=31,k=51,scaled=50")
    got = {mh.ksize: mh for mh in sig.minhashes()}
    assert sorted(got) == [21, 31, 51]
    for k, mh in got.items():
        assert np.array_equal(mh._mins_array(), oracle.sketch_dna_bulk(buf, k, scaled=50, nthreads=4)), k


@pytest.mark.parametrize("moltype", ["protein", "dayhoff", "hp"])
def test_protein_entry_points_equal_oracle(sm, buf, moltype):
    k = 10
    mh = sm.MinHash(0, k, is_protein=moltype == "protein", dayhoff=moltype == "dayhoff", hp=moltype == "hp", scaled=1)
    dna = buf[:30_000].upper().replace(b"N", b"A").decode()
    want = oracle.seq_to_hashes_protein(dna, k, moltype, is_protein=False)
    assert mh.seq_to_hashes(dna) == want.tolist() and len(want) == 2 * (len(dna) - 3 * k + 1)
    mh.add_sequence(dna)                                                          # translated, six frames
    assert np.array_equal(mh._mins_array(), np.unique(want[want != 0]))
    rng = np.random.default_rng(5)
    aa = "".join(rng.choice(list("ACDEFGHIKLMNPQRSTVWY"), size=20_000))
    for ka in (10, 100):                                                          # the register-window and the byte-wise kernel
        pm = sm.MinHash(0, ka, is_protein=moltype == "protein", dayhoff=moltype == "dayhoff", hp=moltype == "hp", scaled=1)
        want = oracle.seq_to_hashes_protein(aa, ka, moltype)
        assert pm.seq_to_hashes(aa, is_protein=True) == want.tolist()
        pm.add_protein(aa)
        assert np.array_equal(pm._mins_array(), np.unique(want[want != 0]))


def _rank_registers(hs, p):
    "regs[h & (2^p - 1)] = max(clz64(h >> p) + 1 - p) over the hashes"
    regs = np.zeros(1 << p, dtype=np.uint8)
    rest = [int(h) >> p for h in hs]
    rank = np.array([64 - v.bit_length() + 1 - p for v in rest], dtype=np.uint8)
    np.maximum.at(regs, (hs & np.uint64((1 << p) - 1)).astype(np.int64), rank)
    return regs


@pytest.mark.parametrize("k", KS)
def test_hll_registers_equal_oracle(sm, buf, k):
    from sourmash_amd.hll import HLL
    p = 12
    part = buf[:120_000]
    h = HLL.from_buffer(b"HLL" + bytes([1, p, 64 - p, k]) + bytes(1 << p))
    h.add_sequence(part, force=True)
    out = np.zeros(len(part) - k + 1, dtype=np.uint64)
    n = oracle.lib().orc_seq_to_hashes_dna(part, len(part), k, 42, 1, oracle._ptr(out))
    hs = out[:n]
    hs = hs[hs != 0]
    assert np.array_equal(np.frombuffer(h.registers(), dtype=np.uint8), _rank_registers(hs, p)), k
