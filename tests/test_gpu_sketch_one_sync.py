"""DeviceSketcher.sketch with the kept count left on the device (smgpu_sketch_dna_raw: kernel, uniform sort, one copy, one
synchronisation; csrc/uniform_sort.hip) against the oracle, with sort_counters() saying which sort served the call: the bucket form
for hashes of random sequence, the one-workgroup form for a small buffer, the general sort after the uniform one has declined
kept hashes that do not spread (one k-mer repeated, a short period).  Poly-A and the period are sketched at scaled = 1: at
scaled = 1000 their one / 150 distinct hashes are most likely not kept at all and nothing would be sorted.  Run with -m gpu."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def smd():
    import torch  # noqa: F401
    import sourmash_amd
    from sourmash_amd import device
    assert sourmash_amd.gpu_available()
    return device


def random_dna(n, seed):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, size=n)]


def sketch_and_path(smd, sk, host):
    import torch
    seq = torch.from_numpy(host.copy()).cuda()
    before = smd.sort_counters()
    got = sk.sketch(seq).cpu().numpy().view(np.uint64)
    after = smd.sort_counters()
    return got, {k: after[k] - before[k] for k in before}


CASES = [
    # name, sequence, scaled, the path
    ("random-2e7-scaled-1000", lambda: random_dna(20_000_000, 1), 1000, "bucket"),
    ("random-2e7-scaled-1", lambda: random_dna(20_000_000, 2), 1, "bucket"),
    ("random-4.6e6-scaled-1000", lambda: random_dna(4_600_000, 3), 1000, "small"),
    ("poly-A-1e6", lambda: np.full(1_000_000, ord("A"), dtype=np.uint8), 1, "fellback"),
    ("period-150-1e7", lambda: np.tile(random_dna(150, 4), 10_000_000 // 150 + 1)[:10_000_000], 1, "fellback"),
]


@pytest.mark.parametrize("name,make,scaled,path", CASES, ids=[c[0] for c in CASES])
def test_sketch_against_the_oracle(smd, name, make, scaled, path):
    host = make()
    sk = smd.DeviceSketcher(ksize=31, scaled=scaled)
    got, took = sketch_and_path(smd, sk, host)
    assert took == {"bucket": int(path == "bucket"), "small": int(path == "small"), "fellback": int(path == "fellback")}, (name, took)
    want = oracle.sketch_dna_bulk(host, 31, scaled=scaled, nthreads=oracle.usable_cpus())
    assert np.array_equal(got, want), (name, len(got), len(want))
    again, _ = sketch_and_path(smd, sk, host)                 # the sketcher's buffers, used a second time
    assert np.array_equal(again, want), name


def test_a_capacity_too_small_is_reported_with_the_true_count_and_retried(smd):
    import torch
    from sourmash_amd._lowlevel import lib
    from sourmash_amd.utils import decode_str
    host = random_dna(300_000, 5)
    seq = torch.from_numpy(host.copy()).cuda()
    mh = oracle.OracleMinHash(0, 31, scaled=100, track_abundance=True)
    mh.add_sequence(host.tobytes())
    kept = int(np.asarray(mh.abunds).sum())
    want = np.asarray(mh.mins, dtype=np.uint64)
    assert kept > 2000
    # the raw call with room for 1,000 hashes: the error names the count, result[0] holds it
    sk = smd.DeviceSketcher(ksize=31, scaled=100)
    sk._reserve(1000)
    assert sk.cap == 1000
    lib.sourmash_err_clear()
    ret = lib.smgpu_sketch_dna_raw(seq.data_ptr(), seq.numel(), 31, 42, sk.max_hash, sk.out.data_ptr(), sk.cap, sk.result.data_ptr(),
                                   sk.ws.data_ptr(), sk.ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert ret == 0xFFFFFFFFFFFFFFFF and lib.sourmash_err_get_last_code() != 0
    message = decode_str(lib.sourmash_err_get_last_message())
    assert "output capacity too small: %d kept hashes > capacity 1000" % kept in message, message
    assert int(sk.result[0].item()) == kept
    lib.sourmash_err_clear()
    # the sketcher: its estimate forced too small, it grows and repeats the call
    sk2 = smd.DeviceSketcher(ksize=31, scaled=100)
    sk2.capacity_for = lambda n_bases: 1000
    got = sk2.sketch(seq).cpu().numpy().view(np.uint64)
    assert sk2.cap == kept + 1024 and int(sk2.result[0].item()) == kept
    assert np.array_equal(got, want)


def test_two_sketchers_on_two_streams_interleaved(smd):
    import torch
    hosts = [random_dna(3_000_000, 6), random_dna(30_000_000, 7)]       # the one-workgroup form and the bucket form
    seqs = [torch.from_numpy(h.copy()).cuda() for h in hosts]
    wants = [oracle.sketch_dna_bulk(h, 31, scaled=1000, nthreads=oracle.usable_cpus()) for h in hosts]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    sks = [smd.DeviceSketcher(ksize=31, scaled=1000), smd.DeviceSketcher(ksize=31, scaled=1000)]
    torch.cuda.synchronize()
    before = smd.sort_counters()
    for rep in range(3):
        gots = [None, None]
        for i in (0, 1, 1, 0):
            with torch.cuda.stream(streams[i]):
                gots[i] = sks[i].sketch(seqs[i]).clone()
        torch.cuda.synchronize()
        for i in (0, 1):
            assert np.array_equal(gots[i].cpu().numpy().view(np.uint64), wants[i]), (rep, i)
    after = smd.sort_counters()
    assert {k: after[k] - before[k] for k in before} == {"bucket": 6, "small": 6, "fellback": 0}
