"""Inputs for the FASTA / FASTQ parser (sourmash_amd/csrc/fastx.hip) and a per-line reference of what it must make of them.

The reference is written from the format statement at the top of fastx.hip, line by line, and knows nothing of lanes, blocks or
masks.  tests/test_fastx_core_cpu.py runs the host emulation of the kernels against it, tests/test_gpu_fastx_edges.py the device.
Every case is deterministic (np.random.default_rng with fixed seeds) and has a name.

The contract is four-line FASTQ: header, sequence, '+' line, quality.  Multi-line FASTQ is NOT the contract; what the reference
says of a FASTQ whose records span more lines is only "lines are counted mod 4", which is also all the device does."""
import functools
from collections import namedtuple

import numpy as np

LANE, WAVE, BLOCK = 32, 2048, 8192
SPANS = 1024                                   # threads of the offsets walk
PIECE_SIZES = (1, 7, 31, 32, 33, 100, 8192, 8193)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def _lines(raw):
    "the lines of raw, split at LF only, each with its LF if it has one; a trailing LF opens no line"
    if not raw:
        return []
    parts = raw.split(b"\n")
    last = parts.pop()
    lines = [p + b"\n" for p in parts]
    if last:
        lines.append(last)
    return lines


def reference(raw, fastq):
    """-> (bytes, record_starts): the compacted stream and, per record, the offset just behind its separator byte.

    FASTA: a line whose first byte is '>' contributes that byte, and a record starts behind it; any other line contributes its
    bytes without CR and LF (a file that does not begin with '>' begins on a sequence line).  FASTQ: line i with i % 4 == 0
    contributes its first byte whatever it is (an empty line's LF included) and a record starts behind it; line i % 4 == 1
    contributes its bytes without CR and LF; the other two contribute nothing.  Multi-line FASTQ is not the contract."""
    raw = bytes(raw)
    out, starts, at = [], [], 0
    for i, line in enumerate(_lines(raw)):
        if (i % 4 == 0) if fastq else line[:1] == b">":
            out.append(line[:1])
            at += 1
            starts.append(at)
        elif (i % 4 == 1) if fastq else True:
            body = line.replace(b"\r", b"").replace(b"\n", b"")
            out.append(body)
            at += len(body)
    return b"".join(out), starts


def reference_carry(raw, fastq):
    """-> (state, ended_on_lf) behind the file.  state: FASTA, the kind of the line the last byte is on (1 sequence, 2 header;
    1 in front of the first byte); FASTQ, the number of the line the last byte is on, mod 4 (3 in front of the first byte)."""
    lines = _lines(bytes(raw))
    if not lines:
        return (3 if fastq else 1), 1
    state = (3 + len(lines)) & 3 if fastq else (2 if lines[-1][:1] == b">" else 1)
    return state, int(lines[-1].endswith(b"\n"))


def records_of(raw, fastq):
    """the reference's stream cut at its separator bytes: the sequences a sketch must see, one add_sequence each (a FASTA that
    begins on a sequence line has a record in front of its first header)"""
    out, starts = reference(raw, fastq)
    recs = [out[:starts[0] - 1]] if starts and starts[0] > 1 else ([] if starts else [out])
    for j, s in enumerate(starts):
        recs.append(out[s:starts[j + 1] - 1 if j + 1 < len(starts) else len(out)])
    return recs


def records_by_splitlines(raw, fastq):
    "the same records read the way a line-oriented host parser would: bytes.splitlines, headers by '>' / every fourth line"
    lines = bytes(raw).splitlines()
    if fastq:
        return [lines[i + 1] if i + 1 < len(lines) else b"" for i in range(0, len(lines), 4)]
    recs, cur = [], None
    for ln in lines:
        if ln[:1] == b">":
            if cur is not None:
                recs.append(cur)
            cur = b""
        else:
            cur = (cur or b"") + ln
    if cur is not None:
        recs.append(cur)
    return recs


# ---- cutting a file into pieces ------------------------------------------------------------------------------------------------------
def cuts_full(n, size):
    "offsets of pieces of `size` bytes over n bytes, with one empty piece in the middle"
    c = list(range(0, n, size)) + [n]
    mid = len(c) // 2
    return np.array(c[:mid + 1] + c[mid:], dtype=np.uint64)


def cuts_windowed(n, size, points, halfwidth=16):
    """the cuts of cuts_full that lie within `halfwidth` bytes of one of `points` (and 0 and n): a coarsening of the full cut --
    every piece still begins at a multiple of `size` -- that keeps the short pieces where they matter.  One piece of `size` bytes is
    the same launch wherever it lies in the file; what differs is the carry that enters it and the bytes around a point."""
    keep = {0, n}
    for p in points:
        lo = max(0, p - halfwidth)
        first = (lo + size - 1) // size * size
        keep.update(range(first, min(n, p + halfwidth) + 1, size))
    c = sorted(keep)
    mid = len(c) // 2
    return np.array(c[:mid + 1] + c[mid:], dtype=np.uint64)


def piece_cuts(case, size, full_from=100):
    """Pieces of `size` bytes and one empty piece in the middle.  A piece of a given size is the same parser run wherever it lies
    in a file: what differs is the carry that enters it and the bytes in it.  5.5 MB of cases in pieces of a few bytes are millions
    of runs, so for sizes below `full_from` a case longer than 256 bytes keeps the cuts only near its points (points_of) -- within
    16 bytes, or two pieces if that is more -- and the stretches between are single pieces that begin and end at multiples of
    `size`.  Sizes from `full_from` on, and short cases, are cut all the way through."""
    n = len(case.raw)
    if n <= 256 or size >= full_from:
        return cuts_full(n, size)
    return cuts_windowed(n, size, points_of(case), max(16, 2 * size))


def points_of(case):
    "where short pieces matter in a case: its event (six spread positions where it has none), the block edges, the end"
    n = len(case.raw)
    own = list(case.points) or [n * k // 7 for k in range(1, 7)]
    return sorted(set(own + list(range(BLOCK, n + 1, BLOCK)) + [n]))


# ---- building blocks ------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name raw fastq points")


def _dna(rng, n):
    return ACGT[rng.integers(0, 4, size=n)].tobytes()


def _fill(rng, length, eol, closed=True, header=True, width=60):
    """exactly `length` bytes of FASTA: a short header line (if there is room), then ACGT lines of about `width` bases ending in
    `eol`; closed: the last line is complete (its LF is the last byte), else the text stops inside a sequence line"""
    e = len(eol)
    a = bytearray(_dna(rng, length))
    at = 0
    if header and length >= 3 + 2 * e + 1:
        a[0:2 + e] = b">s" + eol
        at = 2 + e
    end = length - e if closed else length
    assert not closed or length >= e, (length, eol)
    pos = at + width
    while pos + e <= end - 2:
        a[pos:pos + e] = eol
        pos += width + e
    if closed:
        a[length - e:length] = eol
    return bytes(a)


def _fastq_record(rng, name, r, eol, q0=None, plus=b"+"):
    q = bytearray(rng.integers(33, 74, size=r, dtype=np.uint8).tobytes())
    if q0 is not None and r:
        q[0] = q0
    return b"@" + name + eol + _dna(rng, r) + eol + plus + eol + bytes(q) + eol


POSITIONS = [30, 31, 32, 33] + [WAVE - 2 + i for i in range(4)] + [BLOCK - 2 + i for i in range(4)] + [2 * BLOCK - 2 + i for i in range(4)]
END_N = 20011                                  # the events "at n - 1" and "at n - 2": files of this many bytes that stop right behind the event


def _fasta_event(rng, event, p, eol, final_lf):
    "a FASTA in which the event's LF (for gt_midline: its '>') is byte p, and some more lines behind it"
    e = len(eol)
    tail = b">r2 more" + eol + _dna(rng, 47) + eol + _dna(rng, 13) + (eol if final_lf else b"")
    if event == "lf_header":                   # ...LF at p, '>' at p + 1
        return _fill(rng, p + 1, eol) + tail
    if event == "crlf_pair":                   # CR at p - 1, LF at p, whatever the other line ends are
        return _fill(rng, p - 1, eol, closed=False) + b"\r\n" + _dna(rng, 40) + eol + tail
    if event == "empty_line":                  # a complete line, then a line that holds only its line end: its LF at p
        return _fill(rng, p + 1 - e, eol) + eol + _dna(rng, 40) + eol + tail
    if event == "gt_midline":                  # '>' at p inside a sequence line
        return _fill(rng, p, eol, closed=False) + b">" + _dna(rng, 9) + eol + tail
    raise ValueError(event)


def _fastq_event(rng, kind, p, eol, final_lf):
    "a four-line FASTQ in which the LF that ends a line of `kind` (0 header .. 3 quality) is byte p"
    e = len(eol)
    r = 3 if p < 200 else 20
    out, i = b"", 0
    while len(out) + 400 <= p:                 # whole records in front, of varying length
        out += _fastq_record(rng, b"r%d" % i, int(rng.integers(1, 90)), eol, q0=b"@>+I"[i % 4], plus=b"+r%d" % i if i % 3 == 0 else b"+")
        i += 1
    # the record that holds the event: the name is as long as it takes
    behind_name = e + (r + e if kind >= 1 else 0) + (1 + e if kind >= 2 else 0) + (r + e if kind >= 3 else 0)
    name_len = p + 1 - len(out) - 1 - behind_name
    assert name_len >= 1, (kind, p, eol)
    rec = _fastq_record(rng, (b"x" * name_len), r, eol, q0=ord("@"))
    out += rec
    assert out[p:p + 1] == b"\n" and len(out) - len(rec) + 1 + name_len + behind_name == p + 1
    out += _fastq_record(rng, b"after", 41, eol, q0=ord(">")) + _fastq_record(rng, b"last", 5, eol)
    return out if final_lf else out[:-e]


def _sweep(rng):
    for eol_name, eol in (("lf", b"\n"), ("crlf", b"\r\n")):
        for p in POSITIONS:
            for final_lf in (True, False):
                tag = f"p{p}-{eol_name}-{'lf' if final_lf else 'nolf'}"
                for event in ("lf_header", "crlf_pair", "empty_line", "gt_midline"):
                    yield Case(f"sweep-fasta-{event}-{tag}", _fasta_event(rng, event, p, eol, final_lf), 0, (p,))
                for kind in range(4):
                    yield Case(f"sweep-fastq-line{kind}-{tag}", _fastq_event(rng, kind, p, eol, final_lf), 1, (p,))
        for back in (1, 2):                    # the event's LF at n - 1 and at n - 2: the file stops right behind it
            p = END_N - back
            for event in ("lf_header", "crlf_pair", "empty_line", "gt_midline"):
                raw = _fasta_event(rng, event, p, eol, True)[:p + back]
                yield Case(f"sweep-fasta-{event}-n-{back}-{eol_name}", raw, 0, (p,))
            for kind in range(4):
                raw = _fastq_event(rng, kind, p, eol, True)[:p + back]
                yield Case(f"sweep-fastq-line{kind}-n-{back}-{eol_name}", raw, 1, (p,))


def _no_line_start(rng):
    "a line longer than a lane, a wavefront, a block, two blocks: spans with no line start in them"
    for length in (40, 2100, 8300, 17000):
        for off in (0, 1, BLOCK - 1):
            front = b"" if off == 0 else b"\n" if off == 1 else _fill(rng, off, b"\n")
            hdr = b">" + bytes(rng.integers(33, 127, size=length - 2, dtype=np.uint8).tobytes()) + b"\n"
            yield Case(f"long-header-{length}-at{off}", front + hdr + _dna(rng, 50) + b"\n>z\n" + _dna(rng, 30) + b"\n", 0, (off, off + length))
            yield Case(f"long-sequence-{length}-at{off}", front + _dna(rng, length - 1) + b"\n>z\n" + _dna(rng, 30) + b"\n", 0, (off, off + length))
        q = bytearray(rng.integers(33, 127, size=length - 1, dtype=np.uint8).tobytes())
        raw = b"@long\n" + _dna(rng, length - 1) + b"\n+\n" + bytes(q) + b"\n" + _fastq_record(rng, b"next", 33, b"\n")
        yield Case(f"long-quality-{length}", raw, 1, (6 + length, 6 + 2 * length + 2))


def _many_line_starts(rng):
    for count in (32, 70):
        raw = b">a\n" + _dna(rng, 40) + b"\n" * count + _dna(rng, 40) + b"\n>b\n" + _dna(rng, 20) + b"\n"
        yield Case(f"lfs-{count}-fasta", raw, 0, (43,))
        yield Case(f"lfs-{count}-fastq", b"@a\n" + _dna(rng, 40) + b"\n" * count + _dna(rng, 40) + b"\n+\nIIII\n", 1, (43,))
    for r in (1, 2, 0):
        raw = b"".join(_fastq_record(rng, b"%d" % (i % 10), r, b"\n") for i in range(60))
        yield Case(f"fastq-reads-of-{r}", raw, 1, ())
        yield Case(f"fastq-reads-of-{r}-crlf", b"".join(_fastq_record(rng, b"%d" % (i % 10), r, b"\r\n") for i in range(60)), 1, ())
    for q0 in b"@>+":
        raw = b"".join(_fastq_record(rng, b"q%d" % i, 7 + i % 5, b"\n", q0=q0) for i in range(40))
        yield Case(f"fastq-quality-starts-with-{chr(q0)}", raw, 1, ())
    raw = b"".join(_fastq_record(rng, b"n%d" % i, 11, b"\n", plus=b"+n%d extra" % i) for i in range(40))
    yield Case("fastq-plus-name-lines", raw, 1, ())


def _degenerate(rng):
    for b in (b">", b"@", b"A", b"\n"):
        for fastq in (0, 1):
            yield Case(f"one-byte-{b[0]:02x}-{'fastq' if fastq else 'fasta'}", b, fastq, ())
    yield Case("header-only-fasta", b">only a header", 0, ())
    yield Case("header-only-fasta-lf", b">only a header\n", 0, ())
    yield Case("header-only-fastq", b"@only a header", 1, ())
    yield Case("header-only-fastq-lf", b"@only a header\n", 1, ())
    yield Case("fasta-begins-on-sequence", _dna(rng, 70) + b"\n" + _dna(rng, 30) + b"\n>h\n" + _dna(rng, 45) + b"\n", 0, ())
    yield Case("fasta-ends-inside-header", b">a\n" + _dna(rng, 100) + b"\n>the file stops he", 0, ())
    yield Case("fasta-ends-inside-header-block", _fill(rng, BLOCK - 3, b"\n") + b">stops here", 0, (BLOCK,))
    five = [b"@r1", _dna(rng, 25), b"+", b"I" * 25, b"@r2"]
    for count in (1, 2, 3, 5):
        yield Case(f"fastq-{count}-lines", b"\n".join(five[:count]) + b"\n", 1, ())
        yield Case(f"fastq-{count}-lines-nolf", b"\n".join(five[:count]), 1, ())
    for n in (31, 32, 33, BLOCK - 1, BLOCK, BLOCK + 1):
        yield Case(f"plain-sequence-{n}-fasta", _dna(rng, n), 0, ())
        yield Case(f"plain-sequence-{n}-fastq", _dna(rng, n), 1, ())


def _adversarial(rng):
    "strings over ACGT>@+ CR LF with short lines, at lengths around 32 j and 8,192 j"
    alphabet = np.frombuffer(b"ACGT>@+\r\n", dtype=np.uint8)
    for i in range(200):
        if i < 120:
            n = 32 * int(rng.integers(1, 9)) + int(rng.integers(-2, 3))
        else:
            n = BLOCK * int(rng.integers(1, 4)) + int(rng.integers(-2, 3))
        p_lf = float(rng.choice([0.05, 0.15, 0.4]))
        probs = np.array([1, 1, 1, 1, 0.5, 0.5, 0.5, 0.4, 0], dtype=float)
        probs = probs / probs.sum() * (1 - p_lf)
        probs[8] = p_lf
        raw = alphabet[rng.choice(9, size=n, p=probs)].tobytes()
        yield Case(f"random-{i}-n{n}-{'fastq' if i % 2 else 'fasta'}", raw, i % 2, ())


BIG_N = (SPANS + 1) * BLOCK + 7                # 1,025 blocks and a bit: two blocks per span of the offsets walk


def _big(rng, fastq):
    parts, total, i = [], 0, 0
    eol = b"\n" if fastq else b"\r\n"
    while total < BIG_N:
        L = int(rng.integers(20, 3001))
        name = b"rec%d" % i + (b" " + b"h" * (2 * BLOCK + 600) if i % 50 == 49 else b"")   # every 50th header covers a whole block
        if fastq:
            rec = _fastq_record(rng, name, L, eol, q0=b"@>+I"[i % 4])
        else:
            s = _dna(rng, L)
            rec = b">" + name + eol + eol.join(s[j:j + 80] for j in range(0, L, 80)) + eol
        parts.append(rec)
        total += len(rec)
        i += 1
    return Case(f"blocks-1025-{'fastq' if fastq else 'fasta-crlf'}", b"".join(parts)[:BIG_N], fastq, ())


@functools.lru_cache(maxsize=None)
def small_cases():
    "every case but the two of 1,025 blocks"
    rng = np.random.default_rng(20240917)
    cases = []
    for gen in (_sweep, _no_line_start, _many_line_starts, _degenerate, _adversarial):
        cases.extend(gen(rng))
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def big_cases():
    rng = np.random.default_rng(1025)
    return (_big(rng, 0), _big(rng, 1))


def piece_cases():
    "the cases that are cut into pieces: at most three blocks long"
    return tuple(c for c in small_cases() if len(c.raw) <= 3 * BLOCK)


BIG_CUTS = (BLOCK * SPANS, BLOCK * SPANS + 1)   # the 1,025-block cases in two pieces: 1,024 blocks / 1,024 blocks and a byte first


Expected = namedtuple("Expected", "out starts kept records carry")


def expected_of(raw, fastq):
    "the reference's answer: (bytes, starts as uint64 array, kept, records, (state, ended on LF))"
    out, starts = reference(raw, fastq)
    return Expected(out, np.array(starts, dtype=np.uint64), len(out), len(starts), reference_carry(raw, fastq))


@functools.lru_cache(maxsize=None)
def expected(name):
    "the reference's answer for a case, computed once and shared"
    case = by_name()[name]
    return expected_of(case.raw, case.fastq)


@functools.lru_cache(maxsize=None)
def by_name():
    return {c.name: c for c in small_cases() + big_cases()}


# a dozen files for the entry points users call (tests/test_gpu_fastx_edges.py): real records around one edge each
def named_files():
    rng = np.random.default_rng(12)
    out = {}

    def fasta(front_len, eol, tail):
        return _fill(rng, front_len, eol, width=70) + tail

    seq = lambda n: _dna(rng, n)                                             # noqa: E731
    out["cr-last-in-block.fa"] = fasta(BLOCK + 1, b"\r\n", b">two\r\n" + seq(300) + b"\r\n")         # CR at 8,191, LF at 8,192
    out["gt-first-in-block.fa"] = fasta(BLOCK, b"\n", b">two\n" + seq(300) + b"\n")                   # '>' at 8,192
    out["gt-first-in-block-crlf.fa"] = fasta(2 * BLOCK, b"\r\n", b">two\r\n" + seq(300) + b"\r\n")
    out["header-spans-a-block.fa"] = fasta(BLOCK - 100, b"\n", b">" + b"long name " * 1700 + b"\n" + seq(500) + b"\n>three\n" + seq(90) + b"\n")
    out["no-final-lf.fa"] = fasta(3000, b"\n", b">two\n" + seq(200))
    out["header-only-tail.fa"] = fasta(BLOCK - 5, b"\n", b">tail header and nothing else")
    out["begins-on-sequence.fa"] = seq(100) + b"\n" + seq(50) + b"\n" + fasta(BLOCK + 17, b"\n", b">two\n" + seq(120) + b"\n")
    out["empty-lines-and-gt.fa"] = fasta(BLOCK - 1, b"\n", b"\n\n" + seq(40) + b">" + seq(40) + b"\n\n>two\n" + seq(100) + b"\n\n")
    for phase in range(4):                                                   # bytes 8,191 and 8,192 lie inside line `phase` of a record
        front = b""
        while len(front) <= BLOCK - 600:
            front += _fastq_record(rng, b"f%d" % len(front), int(rng.integers(30, 120)), b"\n")
        name_len = BLOCK - len(front) + 20 if phase == 0 else BLOCK - len(front) - 2 - (phase - 1) * 41 - 20
        rec = b"@" + b"n" * name_len + b"\n" + seq(40) + b"\n+" + b"p" * 39 + b"\n" + b"I" * 40 + b"\n"
        raw = front + rec
        assert b"\n" not in raw[BLOCK - 2:BLOCK + 2] and raw[:BLOCK].count(b"\n") % 4 == phase
        out[f"block-entered-in-phase-{phase}.fq"] = raw + b"".join(_fastq_record(rng, b"m%d" % i, 150, b"\n", q0=b"@>+"[i % 3]) for i in range(70))
    out["fastq-no-final-lf-crlf.fq"] = _fastq_event(rng, 3, 2 * BLOCK - 1, b"\r\n", False)
    return out
