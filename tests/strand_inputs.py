"""Inputs for the checks of the sketch kernel's staged form (tests/test_strand_lds_cpu.py on the host emulation,
tests/test_gpu_strand_lds.py on the GPU): what can go wrong when the tile is staged upper-cased and complemented, validity is
decided per tile, and the strand is picked on the first 8 bytes.  A tile is 4,096 start positions; every input is at most three."""
import numpy as np

TILE = 4096
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s):
    return bytes(s).translate(_COMP)[::-1]


def rand_dna(rng, n, alphabet=b"ACGTacgt"):
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=n))


def tie_kmers(rng, k):
    """k-mers whose first 8 bytes equal those of their reverse complement, X + mid + revcomp(X): `mid` decides, so that the
    forward strand wins once and the reverse complement once; from k = 34 on a pair that ties on the second 8-byte chunk too;
    at even k full palindromes (both strands equal: the forward one is taken)."""
    out = []
    if k >= 17:
        x = rand_dna(rng, 8, b"ACGT")
        m = k - 16
        out += [x + b"A" * m + revcomp(x), x + b"T" * m + revcomp(x)]          # A.. < T..: forward wins; T.. > A..: reverse wins
        if m > 1:
            out += [x + b"C" + b"G" * (m - 1) + revcomp(x), x + b"G" * (m - 1) + b"C" + revcomp(x)]
    if k >= 34:
        x, y = rand_dna(rng, 8, b"ACGT"), rand_dna(rng, 8, b"ACGT")
        m = k - 32
        out += [x + y + b"A" * m + revcomp(y) + revcomp(x), x + y + b"T" * m + revcomp(y) + revcomp(x)]
    if k % 2 == 0:
        h = rand_dna(rng, k // 2, b"ACGT")
        out += [h + revcomp(h), b"AT" * (k // 2)]
    return out


def lengths(k):
    return [k - 1, k, TILE - 1, TILE, TILE + k - 2, TILE + k - 1, 2 * TILE + 5]


def inputs(k, seed=0):
    """name -> bytes.  `random_L` for the lengths of the issue; `n_edges`: N on a tile's first byte, on its last byte and inside
    the next tile's k - 1 byte halo; `separators`: a newline every 150 bytes (every tile dirty); `ties`: the constructed k-mers at
    every position modulo 16, in the first (clean) tile and across the tile boundary."""
    rng = np.random.default_rng(1000 * k + seed)
    out = {}
    for n in lengths(k):
        out[f"random_{n}"] = rand_dna(rng, n)
    s = bytearray(rand_dna(rng, 2 * TILE + 5))
    for i in (TILE, 2 * TILE - 1, 2 * TILE + max(k - 2, 0) // 2, 2 * TILE + max(k - 2, 0)):
        if i < len(s):
            s[i] = ord("N")
    out["n_edges"] = bytes(s)
    s = bytearray(rand_dna(rng, 2 * TILE + 5))
    s[149::150] = b"\n" * len(s[149::150])
    out["separators"] = bytes(s)
    parts, pos = [], 0
    kms = tie_kmers(rng, k)
    for i in range(17 * max(len(kms), 1)):
        pad = rand_dna(rng, 1 + (i % 3), b"ACGT") if kms else rand_dna(rng, 16, b"ACGT")
        parts.append(pad)
        if kms:
            parts.append(kms[i % len(kms)] if i % 5 else kms[i % len(kms)].lower())
    body = b"".join(parts)
    lead = rand_dna(rng, max(0, TILE - len(body) // 2), b"ACGT")           # the run of ties straddles the first tile boundary
    out["ties"] = (body + lead + body + rand_dna(rng, 50, b"ACGT"))[:3 * TILE]
    return out
