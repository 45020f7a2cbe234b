#!/usr/bin/env python3
"""Derives the literal code lengths committed in sourmash_amd/csrc/sigwrite_core.hpp (SW_CODE_LEN).

The sample is one flat signature document of 5,000 uniform hashes below max_hash(scaled=1000) (numpy seed 1), as
Signature::to_json writes it.  Weights: the byte counts of that document x 200, plus 1 for every symbol 0 .. 256 (so that every
byte value and the end-of-block symbol have a code).  Lengths: an optimal length-limited prefix code with the longest code at 15
bits (package-merge), so the Kraft sum is exactly 1.  Prints the 257 lengths as the initialiser of the header's array and the
sizes the table gives against zlib for documents of 1,000 / 5,000 / 50,000 hashes.

usage: python tools/make_sigwrite_table.py
"""
import hashlib
import zlib

import numpy as np

MAX_LEN = 15
HEADER_BITS = 3 + 5 + 5 + 4 + 19 * 3 + 258 * 4      # the block header sigwrite_core.hpp builds (a flat 4-bit code-length code)


def document(n, seed):
    rng = np.random.default_rng(seed)
    max_hash = (1 << 64) // 1000
    mins = sorted(set(int(x) for x in rng.integers(0, max_hash, size=n, dtype=np.uint64)))
    md5 = hashlib.md5(("31" + "".join(map(str, mins))).encode()).hexdigest()
    return ('[{"class":"sourmash_signature","email":"","hash_function":"0.murmur64","filename":"GCF_000005845.2_ASM584v2_genomic.fna.gz",'
            '"name":"NC_000913.3 Escherichia coli str. K-12 substr. MG1655, complete genome","license":"CC0","signatures":[{"num":0,"ksize":31,'
            '"seed":42,"max_hash":%d,"mins":[%s],"md5sum":"%s","molecule":"DNA"}],"version":0.4}]'
            % (max_hash, ",".join(map(str, mins)), md5)).encode()


def package_merge(weights, limit):
    "optimal code lengths with no code longer than `limit` (Larmore & Hirschberg); weights > 0"
    n = len(weights)
    leaves = sorted((w, (i,)) for i, w in enumerate(weights))
    packages = list(leaves)
    for _ in range(limit - 1):
        paired = [(packages[i][0] + packages[i + 1][0], packages[i][1] + packages[i + 1][1]) for i in range(0, len(packages) - 1, 2)]
        packages = sorted(leaves + paired, key=lambda p: p[0])
    lengths = [0] * n
    for _, syms in packages[:2 * n - 2]:
        for s in syms:
            lengths[s] += 1
    return lengths


def main():
    text = document(5000, 1)
    counts = np.bincount(np.frombuffer(text, dtype=np.uint8), minlength=256).astype(np.int64)
    weights = [int(c) * 200 + 1 for c in counts] + [1]
    lengths = package_merge(weights, MAX_LEN)
    assert max(lengths) <= MAX_LEN and min(lengths) >= 1
    assert sum(1 << (MAX_LEN - l) for l in lengths) == 1 << MAX_LEN, "Kraft sum is not 1"
    print("static constexpr uint8_t SW_CODE_LEN[257] = {")
    for i in range(0, 257, 32):
        print("    " + ", ".join(str(l) for l in lengths[i:i + 32]) + ",")
    print("};")
    for n in (1000, 5000, 50000):
        t = document(n, 7)
        bits = HEADER_BITS + sum(lengths[b] for b in t) + lengths[256]
        print("// %6d hashes: %7d text bytes, Huffman-only %7d, zlib level 1 %7d, level 6 %7d"
              % (n, len(t), (bits + 7) // 8, len(zlib.compress(t, 1)), len(zlib.compress(t, 6))))


if __name__ == "__main__":
    main()
