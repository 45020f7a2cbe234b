"""GPU parity of the protein / dayhoff / hp kernels (csrc/protein.hip) on the smallest inputs on which a wrong lane, block, round,
flush, spill, `cap` guard or alignment dispatch shows.  A lane of window_fast_kernel owns the 8 window starts of one aligned word, a
block 256 lanes = 2,048 starts, a launch at most 2,048 blocks, so round r of block b owns the starts [(r * 2048 + b) * 2048, + 2048);
a block stages up to 2,048 kept hashes in LDS and flushes after a round that leaves 1,024 or more.

Most cases go through smgpu_sketch_residues_kernels_raw, the only entry point that takes device pointers (the library's own buffers
are always aligned), called as bench.py calls it.  Expected values come from the CPU oracle alone and every comparison is exact: the
sorted multiset of appended hashes, duplicates kept, against the oracle's hashes with 1 <= h <= max_hash.  Every branch a test is
about is shown to be taken by a precondition on the pointers or on the oracle's per-position hashes.  Run with -m gpu."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

LANE = 8                       # window starts of a lane (RW_P)
BLOCK = 256 * LANE             # window starts of a block
GRID = 2048                    # most blocks of a launch
ROUND = GRID * BLOCK           # window starts of a round: 4,194,304
LDS = 2048                     # kept hashes a block stages (RW_OUT_CAP); a round that leaves LDS / 2 or more is flushed
MAX_K = 256
SENTINEL = 0x5A5A5A5A5A5A5A5A
HF = oracle.HF_BY_MOLTYPE

# window lengths: k / 16 = NB = 0 .. 4 take the register-window kernel, its tail of r = k % 16 bytes covering r = 0, 1 .. 7, 8 and
# above 8; k >= 80 takes the byte-wise kernel.  Every k runs with one alphabet, every alphabet with at least three k.
FAST = [(1, "protein"), (7, "protein"), (8, "hp"), (15, "dayhoff"), (16, "dayhoff"), (17, "hp"), (24, "dayhoff"), (32, "hp"),
        (48, "protein"), (63, "dayhoff"), (64, "hp"), (79, "protein")]
BYTEWISE = [(80, "dayhoff"), (85, "hp"), (255, "protein"), (256, "dayhoff")]
assert {k // 16 for k, _ in FAST} == {0, 1, 2, 3, 4} and all(k // 16 > 4 and k <= MAX_K for k, _ in BYTEWISE)
assert {0, 1, 7, 8, 15} <= {k % 16 for k, _ in FAST}
assert all(sum(m == moltype for _, m in FAST + BYTEWISE) >= 3 for moltype in ("protein", "dayhoff", "hp"))


@pytest.fixture(scope="module")
def env():
    import torch
    import sourmash_amd
    from sourmash_amd._lowlevel import lib
    from sourmash_amd.utils import rustcall
    assert sourmash_amd.gpu_available(), "these tests need a real GPU"
    return torch, lib, rustcall


@pytest.fixture(scope="module")
def sm(env):
    import sourmash_amd
    return sourmash_amd


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
AA20 = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
AA_MIXED = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY" * 3 + b"acdefgwy" + b"*XBZxbz" + b"\x00\xfe", dtype=np.uint8)
DNA_MIXED = np.frombuffer(b"ACGT" * 6 + b"acgt" + b"Nn" + b"R\xfe", dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def content_aa(n):
    "residues, lower case, * X B Z and two bytes outside every alphabet; 0xFE and * on the last byte of the first two blocks"
    s = np.random.default_rng(2000 + n).choice(AA_MIXED, size=n)
    if n >= BLOCK:
        s[BLOCK - 1] = 0xfe
    if n >= 2 * BLOCK:
        s[2 * BLOCK - 1] = ord("*")
    return s.tobytes()


@functools.lru_cache(maxsize=None)
def content_dna(n):
    "bases, lower case, N, two non-base bytes; an N ends the codon of residue 2,047 of frame 0 (the last byte of the first block)"
    s = np.random.default_rng(3000 + n).choice(DNA_MIXED, size=n)
    if n > 3 * BLOCK - 1:
        s[3 * BLOCK - 1] = ord("N")
    return s.tobytes()


@functools.lru_cache(maxsize=None)
def two_rounds_aa():
    "a full round and 5,000 residues of a second one"
    return np.random.default_rng(41).choice(AA20, size=ROUND + 5000).tobytes()


@functools.lru_cache(maxsize=None)
def spill_aa():
    "a full round of random residues, then a homopolymer: every window of the second round's first blocks hashes alike"
    return np.random.default_rng(42).choice(AA20, size=ROUND).tobytes() + b"C" * 20000


@functools.lru_cache(maxsize=None)
def two_rounds_dna():
    s = np.random.default_rng(43).choice(np.frombuffer(b"ACGT" * 12 + b"acgtN", dtype=np.uint8), size=2_100_000)
    return s.tobytes()


def frame_residues(n, frame):
    return len(range(frame, n - 2, 3))             # codons starting at frame, frame + 3, ... that end inside the input


def translated_len(n):
    "six segments (frame 0 forward, frame 0 reverse, frame 1 forward, ...), a separator byte after each"
    return 2 * sum(frame_residues(n, f) for f in (0, 1, 2)) + 6


def separators(n):
    "positions of the six separator bytes in the translated buffer"
    pos, at = [], 0
    for s in range(6):
        at += frame_residues(n, s >> 1) + 1
        pos.append(at - 1)
    return pos


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=6)
def oracle_hashes(data, k, moltype, translate, seed=42):
    "one hash per window in the oracle's order (residue input: by start position)"
    h = oracle.seq_to_hashes_protein(data, k, moltype, seed=seed, is_protein=not translate)
    h.setflags(write=False)
    return h


def kept_mask(h, scaled):
    return (h >= 1) & (h <= np.uint64(oracle.max_hash_for_scaled(scaled)))


def want_appended(data, k, moltype, translate, scaled, seed=42):
    h = oracle_hashes(data, k, moltype, translate, seed)
    return np.sort(h[kept_mask(h, scaled)])


def window_exists(n, k, translate):
    return n >= (3 * k if translate else k)


def assert_sub_multiset(got, want):
    u, c = np.unique(got, return_counts=True)
    wu, wc = np.unique(want, return_counts=True)
    idx = np.minimum(np.searchsorted(wu, u), len(wu) - 1)
    assert np.array_equal(wu[idx], u), "a hash the oracle does not keep"
    assert (c <= wc[idx]).all(), "a hash more often than the oracle keeps it"


# ---- the raw entry point ---------------------------------------------------------------------------------------------------------------
def device_view(torch, data, off):
    "data on the device, its first byte `off` bytes behind a 16-byte boundary (an empty tensor has no address: torch gives 0)"
    base = torch.zeros(len(data) + 32, dtype=torch.uint8, device="cuda")
    view = base[off:off + len(data)]
    if len(data):
        view.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
        assert view.data_ptr() % 16 == off
    return view


def aa_view(torch, n_aa, off):
    "room for n_aa residues `off` bytes behind a 16-byte boundary, large enough for the capacity check at every offset"
    need = (n_aa + 7) & ~7
    base = torch.full((need + 32,), 0xEE, dtype=torch.uint8, device="cuda")
    view = base[off:]
    assert view.data_ptr() % 16 == off and view.numel() >= need
    return view


class Raw:
    "one call of smgpu_sketch_residues_kernels_raw: d_count zeroed, d_out and 16 words behind `cap` filled with a sentinel"

    def __init__(self, env, data, k, moltype, translate, scaled, seed=42, seq_off=0, aa_off=0, cap=None, aa_capacity=None):
        torch, lib, rustcall = env
        self.n_aa = translated_len(len(data)) if translate else len(data)
        self.seq = device_view(torch, data, seq_off)
        self.aa = aa_view(torch, self.n_aa, aa_off)
        self.cap = max(self.n_aa, 1) if cap is None else cap
        self.out = torch.full((self.cap + 16,), SENTINEL, dtype=torch.int64, device="cuda")
        self.cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        capacity = self.aa.numel() if aa_capacity is None else aa_capacity
        self.call = lambda: rustcall(lib.smgpu_sketch_residues_kernels_raw, p(self.seq), len(data), k, HF[moltype], seed,
                                     oracle.max_hash_for_scaled(scaled), translate, p(self.aa), capacity, p(self.out), self.cap,
                                     p(self.cnt), stream)
        self.sync = torch.cuda.synchronize
        sp, ap = self.seq.data_ptr(), self.aa.data_ptr()
        # what protein.hip's launchers decide from the pointers
        self.kernels = {"residues_uint4": (sp | ap) % 16 == 0, "translate_words": (sp | ap) % 4 == 0,
                        "window_fast": ap % 8 == 0 and k // 16 <= 4}

    def launch(self):
        ret = self.call()
        self.sync()
        return ret

    def count(self):
        self.sync()
        assert int(self.cnt[1].item()) == 0
        return int(self.cnt[0].item())

    def written(self):
        "d_out and the sentinel words behind it, as the call left them"
        self.sync()
        return self.out.cpu().numpy().view(np.uint64)

    def untouched(self):
        return self.count() == 0 and bool((self.written() == np.uint64(SENTINEL)).all())

    def appended(self):
        "every hash the kernels appended (duplicates kept), sorted; nothing written past them"
        assert self.launch() == self.n_aa
        kept, out = self.count(), self.written()
        assert kept <= self.cap
        assert (out[kept:] == np.uint64(SENTINEL)).all()
        return np.sort(out[:kept])


def scaled_for(n, long_from):
    "every window kept on the short inputs (a single window must show); about 256 a block on the long ones"
    return 1 if n < long_from else 8


def residue_lengths(k):
    return sorted({0, k - 1, k, k + 1, 7, 8, 9, 15, 16, 17, BLOCK - 1, BLOCK, BLOCK + 1, BLOCK + k - 1, BLOCK + k, 2 * BLOCK + 5})


def dna_lengths(k):
    "3 * 2047 .. 3 * 2050 bases: segments of about a block, so that the six separators move across a block seam"
    return sorted(set(range(0, 21)) | {3 * k - 1, 3 * k, 3 * k + 1, 3 * k + 2} | set(range(3 * BLOCK - 3, 3 * BLOCK + 7)))


def check_appended(env, data, k, moltype, translate, scaled, **kw):
    want = want_appended(data, k, moltype, translate, scaled, kw.get("seed", 42))
    assert (len(want) > 0) == window_exists(len(data), k, translate), len(data)
    raw = Raw(env, data, k, moltype, translate, scaled, **kw)
    got = raw.appended()
    assert np.array_equal(got, want), (len(data), k, moltype, translate, kw)
    return raw


# ---- 1. alignment dispatch ---------------------------------------------------------------------------------------------------------------
# (d_seq, d_aa) bytes behind a 16-byte boundary: each of residues_kernel's, translate_launch's and residue_windows_launch's
# conditions on both sides, with the other pointer aligned and with both off
OFFSET_PAIRS = [(0, 0), (1, 0), (4, 0), (15, 0), (0, 1), (0, 4), (0, 8), (4, 4), (4, 8), (15, 1)]


@pytest.mark.parametrize("translate", [False, True], ids=["residues", "dna"])
@pytest.mark.parametrize("k,moltype", [(7, "protein"), (17, "dayhoff"), (85, "hp")])
def test_alignment_dispatch(env, k, moltype, translate):
    if translate:
        lengths = sorted(set(range(0, 21)) | {3 * k + 1, 3 * BLOCK - 1, 3 * BLOCK + 6})
        long_from, content = 3 * BLOCK - 3, content_dna
    else:
        lengths = sorted({k, 15, 16, 17, 33, BLOCK + 1, 2 * BLOCK + 5})
        long_from, content = BLOCK - 1, content_aa
    taken = set()
    for seq_off, aa_off in OFFSET_PAIRS:
        for n in lengths:
            raw = check_appended(env, content(n), k, moltype, translate, scaled_for(n, long_from), seq_off=seq_off, aa_off=aa_off)
            if n:
                taken |= set(raw.kernels.items())
    first = "translate_words" if translate else "residues_uint4"
    assert {(first, True), (first, False)} <= taken
    if k // 16 <= 4:
        assert {("window_fast", True), ("window_fast", False)} <= taken
    else:
        assert ("window_fast", True) not in taken


# ---- 2. and 3. lengths, window lengths, alphabets, seeds -----------------------------------------------------------------------------
@pytest.mark.parametrize("k,moltype", FAST + BYTEWISE)
def test_residue_lengths(env, k, moltype):
    for n in residue_lengths(k):
        raw = check_appended(env, content_aa(n), k, moltype, False, scaled_for(n, BLOCK - 1))
        assert raw.kernels["window_fast"] == (k <= 79) and raw.kernels["residues_uint4"]


@pytest.mark.parametrize("k,moltype", FAST + BYTEWISE)
def test_dna_lengths(env, k, moltype):
    for n in dna_lengths(k):
        raw = check_appended(env, content_dna(n), k, moltype, True, scaled_for(n, 3 * BLOCK - 3))
        assert raw.kernels["window_fast"] == (k <= 79) and raw.kernels["translate_words"]
        if n < 3:
            assert raw.n_aa == 6


def test_dna_lengths_put_separators_on_both_sides_of_a_block_seam():
    "the lengths above: a separator is the last byte of a block, the first byte of the next, and neither"
    at = {p % BLOCK for n in range(3 * BLOCK - 3, 3 * BLOCK + 7) for p in separators(n)}
    assert {BLOCK - 1, 0, 1, BLOCK - 2} <= at
    assert separators(3 * BLOCK - 3)[0] == BLOCK - 1 and separators(3 * BLOCK)[0] == BLOCK


@pytest.mark.parametrize("k,moltype", [(7, "protein"), (85, "hp")])
def test_seeds(env, k, moltype):
    "the oracle's entry point carries the seed in 64 bits (orc_seq_to_hashes_protein, orc_hash_murmur): one seed above 2^32 as well"
    for seed in (0, 1, 2**32 - 1, 2**40 + 12345):
        check_appended(env, content_aa(2 * BLOCK + 5), k, moltype, False, 8, seed=seed)
        check_appended(env, content_dna(3 * BLOCK + 1), k, moltype, True, 8, seed=seed)
    a = want_appended(content_aa(2 * BLOCK + 5), k, moltype, False, 8, seed=1)
    b = want_appended(content_aa(2 * BLOCK + 5), k, moltype, False, 8, seed=2**32 + 1)
    assert not np.array_equal(a, b)                                  # the high half of the seed matters to the expected value


@pytest.mark.parametrize("translate", [False, True], ids=["residues", "dna"])
@pytest.mark.parametrize("k", [0, MAX_K + 1])
def test_window_length_out_of_range_raises_and_writes_nothing(env, k, translate):
    from sourmash_amd.exceptions import SourmashError
    for n in (2, 5000):
        raw = Raw(env, content_dna(n) if translate else content_aa(n), k, "protein", translate, 1)
        with pytest.raises((SourmashError, ValueError)):
            raw.launch()
        assert raw.untouched()


# ---- 4. the round loop, the mid-loop flush, the spill branch and `cap` --------------------------------------------------------------------
def kept_per_block(mask):
    "kept windows of each block of the first round (residue input: the oracle's order is the start position)"
    assert len(mask) >= ROUND
    return np.add.reduceat(mask[:ROUND].astype(np.int64), np.arange(0, ROUND, BLOCK))


def lanes(n_aa, k):
    return (n_aa - k + 1 + LANE - 1) // LANE


def test_second_round_and_mid_loop_flush(env):
    data, k, scaled = two_rounds_aa(), 7, 2
    mask = kept_mask(oracle_hashes(data, k, "protein", False), scaled)
    per_block = kept_per_block(mask)
    assert GRID * 256 < lanes(len(data), k) <= 2 * GRID * 256               # two rounds
    assert 0 < len(mask) - ROUND < 3 * BLOCK and mask[ROUND:].any()        # the second populated in three blocks only
    assert (per_block >= LDS // 2).sum() > GRID // 4                        # these blocks flush between the rounds ...
    assert (per_block < LDS // 2).sum() > GRID // 4                         # ... these do not
    assert per_block.max() < LDS                                            # (no block spills in round 0)
    raw = check_appended(env, data, k, "protein", False, scaled)
    assert raw.kernels["window_fast"] and raw.count() > 2_000_000


def spill_preconditions():
    data, k, scaled = spill_aa(), 7, 4
    h = oracle_hashes(data, k, "protein", False)
    mask = kept_mask(h, scaled)
    per_block = kept_per_block(mask)
    assert per_block.min() >= 1 and per_block.max() <= LDS // 2 - 1         # round 0: something staged, nothing flushed
    homopolymer = oracle.hash_murmur("C" * k)
    assert homopolymer == 237964887603322937 <= oracle.max_hash_for_scaled(scaled)
    assert (h[ROUND:] == np.uint64(homopolymer)).all() and len(h) - ROUND == 20000 - k + 1
    # round 1, block 0: its 2,048 windows are all kept on top of what round 0 left in LDS
    assert per_block[0] + BLOCK > LDS and lanes(len(data), k) > GRID * 256
    return data, k, scaled, homopolymer


def test_spill_past_the_lds_stage(env):
    data, k, scaled, homopolymer = spill_preconditions()
    want = want_appended(data, k, "protein", False, scaled)
    assert int((want == np.uint64(homopolymer)).sum()) == 19994
    raw = check_appended(env, data, k, "protein", False, scaled)
    assert raw.kernels["window_fast"]


@pytest.mark.parametrize("seq_off", [0, 1])
def test_translated_two_rounds(env, seq_off):
    "the benchmark's configuration (protein, k = 10, scaled = 200) over more than one round of translated residues"
    data, k = two_rounds_dna(), 10
    assert lanes(translated_len(len(data)), k) > GRID * 256 and translated_len(len(data)) > ROUND + 8
    raw = check_appended(env, data, k, "protein", True, 200, seq_off=seq_off)
    assert raw.kernels["window_fast"] and raw.kernels["translate_words"] == (seq_off == 0)


@pytest.mark.parametrize("case", ["fast", "bytewise", "spill"])
def test_cap_below_the_kept_count(env, case):
    if case == "spill":
        data, k, scaled, _ = spill_preconditions()
        moltype = "protein"
    else:
        data, scaled = content_aa(2 * BLOCK + 5), 8
        k, moltype = {"fast": (7, "protein"), "bytewise": (85, "dayhoff")}[case]
    want = want_appended(data, k, moltype, False, scaled)
    cap = len(want) // 2
    assert cap > 16
    raw = Raw(env, data, k, moltype, False, scaled, cap=cap)
    assert raw.kernels["window_fast"] == (case != "bytewise")
    assert raw.launch() == len(data)
    assert raw.count() == len(want)                                         # every kept hash is counted ...
    out = raw.written()
    assert_sub_multiset(out[:cap], want)                                    # ... the first `cap` are stored ...
    assert (out[cap:] == np.uint64(SENTINEL)).all() and len(out) == cap + 16    # ... and nothing behind them


@pytest.mark.parametrize("translate", [False, True], ids=["residues", "dna"])
def test_aa_capacity(env, translate):
    from sourmash_amd.exceptions import SourmashError
    data = content_dna(3 * BLOCK + 1) if translate else content_aa(BLOCK + 1)
    n_aa = translated_len(len(data)) if translate else len(data)
    need = (n_aa + 7) & ~7
    assert need > n_aa                                                       # (the whole last word counts, not the residues)
    for short in (need - 1, n_aa, 0):
        raw = Raw(env, data, 7, "protein", translate, 8, aa_capacity=short)
        with pytest.raises((SourmashError, ValueError)):
            raw.launch()
        assert raw.untouched()
    check_appended(env, data, 7, "protein", translate, 8, aa_capacity=need)


# ---- 5. the object API: the retry with a larger `cap`, the dense form ----------------------------------------------------------------------
def _mh(sm, moltype, k, **kw):
    return sm.MinHash(0, k, is_protein=moltype == "protein", dayhoff=moltype == "dayhoff", hp=moltype == "hp", **kw)


def first_cap(n_windows, max_hash):
    "the room DeviceCtx::protein_sketch_host gives its first attempt: 1.5 x the expected kept count + 8 sigma + 4,096"
    expect = n_windows * (max_hash / 2.0**64)
    return min(int(expect * 1.5 + 8.0 * (expect + 1.0) ** 0.5) + 4096, n_windows)


@pytest.mark.parametrize("moltype,k,letter,encoded,scaled", [("protein", 7, "C", "C", 16), ("dayhoff", 16, "C", "a", 4),
                                                             ("hp", 42, "G", "h", 4)])
def test_retry_when_more_is_kept_than_expected(sm, moltype, k, letter, encoded, scaled):
    """a homopolymer whose one hash is kept: every window lands, far beyond what the threshold lets expect, so the first attempt's
    count exceeds its `cap` and the second runs.  (MinHash takes the window length in residues: 7 is the stored ksize 21.)"""
    n = 20000
    h = oracle.hash_murmur(encoded * k)
    assert 1 <= h <= oracle.max_hash_for_scaled(scaled)
    assert n - k + 1 > first_cap(n - k + 1, oracle.max_hash_for_scaled(scaled))
    want = oracle.OracleMinHash(0, 3 * k, scaled=scaled, hash_function=HF[moltype], track_abundance=True)
    want.add_protein(letter * n)
    assert want.mins.tolist() == [h] and want.abunds.tolist() == [n - k + 1]
    if moltype == "protein":
        assert (h, n - k + 1) == (237964887603322937, 19994)
    mh = _mh(sm, moltype, k, scaled=scaled, track_abundance=True)
    mh.add_protein(letter * n)
    assert dict(mh.hashes) == {h: n - k + 1}
    assert mh.md5sum() == want.md5sum()


@pytest.mark.parametrize("k,moltype", [(7, "protein"), (7, "hp"), (85, "dayhoff")])
def test_dense_form(sm, k, moltype):
    "seq_to_hashes: one hash per window in the oracle's order; for DNA the windows that straddle a separator are cut on the host"
    mh = _mh(sm, moltype, k, scaled=1)
    for n in (BLOCK - 1, BLOCK, BLOCK + 1 + k):
        want = oracle.seq_to_hashes_protein(content_aa(n), k, moltype).tolist()
        assert len(want) == n - k + 1 and all(want)
        assert mh.seq_to_hashes(content_aa(n), is_protein=True) == want, n
    for n in [3 * k, 3 * k + 1, 3 * k + 2] + list(range(3 * BLOCK - 3, 3 * BLOCK + 7)):
        want = oracle.seq_to_hashes_protein(content_dna(n), k, moltype, is_protein=False).tolist()
        assert len(want) == 2 * sum(frame_residues(n, f) - k + 1 for f in (0, 1, 2)) and all(want)
        assert mh.seq_to_hashes(content_dna(n)) == want, n
        assert mh.seq_to_hashes(content_dna(n), force=True, bad_kmers_as_zeroes=True) == [0] + want + [0], n
