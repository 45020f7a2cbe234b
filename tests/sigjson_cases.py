"""Inputs for the signature JSON array parser (sourmash_amd/csrc/sigjson.hip) and a reference of what it must make of them.

The reference is written from the documented rules with regular expressions and Python integers, and knows nothing of tiles,
chunks, lanes or look-ahead.  tests/test_sigjson_core_cpu.py runs the host emulation of the kernels against it,
tests/test_gpu_sigjson_edges.py the device.  Every case is deterministic and has a name that says what it is.

The contract, checked by check_block for the emulation and for the device alike:
  (a) an array the parser does not flag is plain (ref_array); its n_values values equal the reference's exactly, and so does n_kept
  (b) a plain array in which every stretch between two neighbouring separators (array start, commas, array end) is at most 63
      bytes is NOT flagged: such a stretch always ends inside the look-ahead.  A plain array with a longer stretch may be flagged
      (it goes to the host parser): those cases carry may_fall_back, and the tagged set is asserted to be the set this rule gives
  (c) the span records and the document flag are the reference's (ref_spans), found or not found, odd or not
Leading zeros ("007", twenty zeros) are plain here, as they are for the host loader, although they are not JSON."""
import functools
import re
import zlib
from collections import namedtuple

import numpy as np

U64 = 2 ** 64 - 1
KM = 9223372036854776                          # max_hash of scaled = 2000 (2^64 / 2000 in f64, as the loaders compute it): the keep_max of most cases
CHUNK, AHEAD, MAX_SPANS, TEXT_PAD = 4096, 64, 8, 16
MINS, ABUND = 0, 1
DOC_ODD = 0x80000000
SPAN = np.dtype([("begin", "<u8"), ("end", "<u8"), ("n_values", "<u4"), ("kind", "<u4"), ("flags", "<u4"), ("pad", "<u4")])
JOB = np.dtype([("text_off", "<u8"), ("len", "<u8"), ("value_off", "<u8"), ("n_values", "<u8")])
PARSED = np.dtype([("n_kept", "<u4"), ("flags", "<u4")])
GUARD = 0xA5A5A5A5A5A5A5A5

Case = namedtuple("Case", "name doc keep_max align behind last may_fall_back json_fix")
RefSpan = namedtuple("RefSpan", "begin end kind n_values odd")
RefArray = namedtuple("RefArray", "plain values n_kept long_stretch")
Expected = namedtuple("Expected", "spans doc_odd arrays")       # arrays: one RefArray per `mins` span, in order


# ---- the reference ----------------------------------------------------------------------------------------------------------------
_KEY = re.compile(rb'"(mins|abundances)"[ \n\r\t]*:[ \n\r\t]*\[')
_PLAIN = re.compile(rb"^[ \n\r\t]*(\d{1,20}[ \n\r\t]*(,[ \n\r\t]*\d{1,20}[ \n\r\t]*)*)?$")


def ref_spans(doc):
    """-> ([RefSpan], document odd).  Every `"mins"` / `"abundances"` key followed by ws* : ws* [ opens an array that runs to the
    first `]`.  n_values = commas + 1 if the array holds a digit, else 0; it is odd if it holds a byte outside digits, commas and
    the four white-space bytes, or commas without digits.  The document is odd (and the scan ends) at an array without a closing
    bracket and at the ninth array."""
    doc = bytes(doc)
    spans, pos = [], 0
    while True:
        m = _KEY.search(doc, pos)
        if m is None:
            return spans, False
        begin = m.end()
        end = doc.find(b"]", begin)
        if end < 0 or len(spans) == MAX_SPANS:
            return spans, True
        body = doc[begin:end]
        commas, has_digit = body.count(b","), re.search(rb"\d", body) is not None
        odd = re.search(rb"[^0-9, \n\r\t]", body) is not None or (commas > 0 and not has_digit)
        spans.append(RefSpan(begin, end, MINS if m.group(1) == b"mins" else ABUND, commas + 1 if has_digit else 0, odd))
        pos = end + 1


def ref_array(body, keep_max):
    """-> (plain, values, n_kept).  Plain: ws*(\\d{1,20} ws*(, ws*\\d{1,20} ws*)*)?, every value <= 2^64 - 1, strictly ascending."""
    body = bytes(body)
    if _PLAIN.match(body) is None:
        return False, [], 0
    values = [int(tok) for tok in body.split(b",")] if body.strip(b" \n\r\t") else []
    plain = all(v <= U64 for v in values) and all(a < b for a, b in zip(values, values[1:]))
    return plain, values, sum(v <= keep_max for v in values)


def longest_stretch(body):
    "the longest run of bytes between two neighbouring separators: array start, commas, array end"
    return max(len(part) for part in bytes(body).split(b","))


@functools.lru_cache(maxsize=None)
def expected(name):
    case = by_name()[name]
    spans, doc_odd = ref_spans(case.doc)
    arrays = []
    for sp in spans:
        if sp.kind == MINS:
            body = case.doc[sp.begin:sp.end]
            arrays.append(RefArray(*ref_array(body, case.keep_max), longest_stretch(body) > AHEAD - 1))
    return Expected(spans, doc_odd, arrays)


def takeable(name):
    "the reference's word on a document the device parser MUST take: nothing odd, every `mins` array plain with short stretches"
    e = expected(name)
    return not e.doc_odd and not any(s.odd for s in e.spans) and all(a.plain and not a.long_stretch for a in e.arrays)


def computed_may_fall_back(name):
    "the 63-byte rule: a document with nothing odd whose `mins` arrays are all plain and one of them has a longer stretch"
    e = expected(name)
    return (not e.doc_odd and not any(s.odd for s in e.spans) and all(a.plain for a in e.arrays) and any(a.long_stretch for a in e.arrays))


# ---- builders ---------------------------------------------------------------------------------------------------------------------
def tokens_of_len(length, maxd=20, start=0):
    "ascending decimal tokens without white space that, joined by commas, are exactly `length` bytes; none longer than maxd digits"
    if length == 0:
        return []
    n = -(-(length + 1) // (maxd + 1))
    base, extra = divmod(length - (n - 1), n)
    digs = [base] * (n - extra) + [base + 1] * extra
    toks = [str(10 ** (d - 1) + start + k) for k, d in enumerate(digs)]
    assert len(",".join(toks)) == length and all(len(t) == d for t, d in zip(toks, digs))
    return toks


def body_of_len(length):
    """a plain array of exactly `length` bytes built from 1- to 20-digit values: one value of every digit count 1 .. 19, then 19-
    and 20-digit values, the last value's digits making up the exact length (no white space anywhere)"""
    if length < 700:
        return ",".join(tokens_of_len(length)).encode()
    ramp = ",".join(str(10 ** (d - 1) + d) for d in range(1, 20)) + ","
    body = (ramp + ",".join(tokens_of_len(length - len(ramp), start=100))).encode()
    assert len(body) == length
    return body


def mins_doc(body, front=b'{"mins":[', back=b"]}"):
    return front + (body if isinstance(body, bytes) else body.encode()) + back


def _case(name, doc, keep_max=KM, align=None, behind=b"", last=False, may_fall_back=False, json_fix=b""):
    return Case(name, bytes(doc), keep_max, zlib.crc32(name.encode()) % 16 if align is None else align % 16, behind, last, may_fall_back, json_fix)


SWEEP_VARIANTS = ("d20", "d19", "d1", "d20-d1-d19")


def seam_body(comma_at, variant):
    """`comma_at` bytes of ascending values of at most 18 digits, a comma at byte `comma_at`, then: a 20-digit value (d20), a
    19-digit value (d19), a 1-digit value (d1: it descends, so the array is not plain) or the three in that order, and two or
    three values more"""
    prefix = ",".join(tokens_of_len(comma_at, maxd=18))
    tail = {"d20": [10 ** 19 + 5, 10 ** 19 + 6, U64], "d19": [10 ** 18 + 5, 10 ** 19 + 1, U64], "d1": [7, 10 ** 19 + 1, U64],
            "d20-d1-d19": [10 ** 19 + 5, 7, 10 ** 18 + 5, U64]}[variant]
    return (prefix + "," + ",".join(map(str, tail))).encode()


def _sizes():
    for n in (0, 1, 63, 64, 65, 4095, 4096, 4097, 4159, 4160, 4161, 8191, 8192, 8193, 12289):
        yield _case(f"size-{n}-bytes", mins_doc(body_of_len(n)))


def _sweeps():
    for seam in (64, 4032, 4096, 8192):
        for d in range(-22, 3):
            for v in SWEEP_VARIANTS:
                yield _case(f"sweep-comma-at-{seam}{d:+d}-{v}", mins_doc(seam_body(seam + d, v)))


def _look_ahead():
    # a comma at the chunk's last byte, white space, a 20-digit value whose last digit is byte `last`: the stretch is last - 4095
    for last in (4157, 4158, 4159, 4160, 4161):
        ws = last - 4095 - 20
        body = ",".join(tokens_of_len(4095, maxd=18)) + "," + " " * ws + str(U64 - 3)
        yield _case(f"last-digit-at-{last}-behind-comma-at-4095", mins_doc(body), may_fall_back=last - 4095 > 63)
    # the same with another value behind it
    for last in (4158, 4159):
        ws = last - 4095 - 20
        body = ",".join(tokens_of_len(4095, maxd=18)) + "," + " " * ws + str(U64 - 3) + "," + str(U64)
        yield _case(f"last-digit-at-{last}-behind-comma-at-4095-one-more-value", mins_doc(body), may_fall_back=last - 4095 > 63)


def _alignment():
    for align in range(16):
        for d in (-20, -1, 0):
            yield _case(f"align-{align}-comma-at-4096{d:+d}-d20", mins_doc(seam_body(4096 + d, "d20")), align=align)
        yield _case(f"align-{align}-size-4161-bytes", mins_doc(body_of_len(4161)), align=align)
        yield _case(f"align-{align}-size-65-bytes", mins_doc(body_of_len(65)), align=align)


def _end_of_block():
    # the array's `]` stands k bytes in front of the end of the whole text block; the array's end address is 1 (mod 16), so that
    # the last line the parser loads reaches 15 bytes past the array
    for n in (100, 4100):
        for k in (1, 2, 15, 16, 17):
            doc = mins_doc(body_of_len(n), back=b"]" + (b"}" + b" " * 16)[:k - 1])
            yield _case(f"end-of-block-array-of-{n}-ends-{k}-bytes-before-it", doc, align=1 - n, last=True, json_fix=b"" if k > 1 else b"}")


LIMIT_VALUES = (("u64-max", str(U64)), ("2^64", str(2 ** 64)), ("2^64+9", str(2 ** 64 + 9)), ("u64-max-6", "18446744073709551609"),
                ("2^64+4-last-digit-0", "18446744073709551620"), ("1999..9", "19999999999999999999"), ("9999..9", "99999999999999999999"),
                ("21-digits", str(10 ** 20)), ("20-zeros", "0" * 20), ("007", "007"), ("u64-max-div-10", "1844674407370955161"))


def _limit():
    for label, x in LIMIT_VALUES:
        yield _case(f"limit-{label}-alone", mins_doc(x), keep_max=U64)
        yield _case(f"limit-{label}-first", mins_doc(f"{x},{U64}"), keep_max=U64)
        yield _case(f"limit-{label}-middle", mins_doc(f"1,{x},{U64}"), keep_max=U64)
        yield _case(f"limit-{label}-last", mins_doc(f"1,2,{x}"), keep_max=U64)
        yield _case(f"limit-{label}-across-byte-4096", mins_doc(",".join(tokens_of_len(4086, maxd=18)) + "," + x), keep_max=U64)
    yield _case("limit-u64-max-with-keep-max-u64-max", mins_doc(f"5,{U64 - 1},{U64}"), keep_max=U64)
    yield _case("limit-u64-max-with-keep-max-of-scaled-2000", mins_doc(f"5,{KM},{U64 - 1},{U64}"))


def _ordered(n):
    return [10 ** 16 + 1000 * i for i in range(n)]                  # 17 digits, 18 bytes a value


def _order():
    n = 300
    cross = CHUNK // 18                                             # value `cross` begins in front of byte 4096, the next one behind it
    assert cross * 18 < CHUNK <= (cross + 1) * 18
    for label, j in (("0-1", 0), ("63-64", 63), ("64-65", 64), ("n-2-n-1", n - 2), ("across-a-chunk", cross)):
        v = _ordered(n)
        v[j + 1] = v[j]
        yield _case(f"order-equal-pair-at-{label}", mins_doc(",".join(map(str, v))))
        v = _ordered(n)
        v[j], v[j + 1] = v[j + 1], v[j]
        yield _case(f"order-descending-pair-at-{label}", mins_doc(",".join(map(str, v))))
    yield _case("order-ascending-300-values", mins_doc(",".join(map(str, _ordered(n)))))
    yield _case("order-single-value", mins_doc("12345"))
    yield _case("order-two-values-equal", mins_doc("5,5"))
    yield _case("order-two-values-descending", mins_doc("6,5"))
    for label, vals in (("keep-max-exactly-last", [5, KM - 1, KM]), ("keep-max-plus-1-last", [5, KM - 1, KM + 1]), ("keep-max-minus-1-last", [5, KM - 2, KM - 1]),
                        ("keep-max-minus-1-exactly-plus-1", [5, KM - 1, KM, KM + 1, U64]), ("all-above-keep-max", [KM + 1, KM + 2]),
                        ("keep-max-at-value-63-of-130", list(range(1, 64)) + [KM] + [KM + 1 + i for i in range(66)]),
                        ("keep-max-at-value-64-of-130", list(range(1, 65)) + [KM] + [KM + 1 + i for i in range(65)])):
        yield _case(f"order-{label}", mins_doc(",".join(map(str, vals))))
    yield _case("order-keep-max-exactly-in-the-middle-all-below-twice-keep-max", mins_doc(f"5,{KM - 1},{KM},{KM + 1},{2 * KM - 2}"))
    yield _case("order-keep-max-u64-max-keeps-all", mins_doc(f"1,{KM},{KM + 1},{U64}"), keep_max=U64)
    yield _case("order-keep-max-0-keeps-only-0", mins_doc("0,1,2"), keep_max=0)


def _separators():
    for label, body in (("trailing-comma", "1,2,"), ("leading-comma", ",1"), ("double-comma", "1,,2"), ("space-for-comma", "1 2"), ("one-space", " "),
                        ("empty", ""), ("newlines-around-values", "\n1\n,\n2\n"), ("all-four-white-space-bytes", " \n\r\t1 \n\r\t, \n\r\t2 \n\r\t"),
                        ("only-commas", ",,"), ("float", "1.0,2"), ("minus", "-1,2"), ("exponent", "1e3,2000"), ("plus", "+1,2"), ("letter", "1,x,3"),
                        ("letter-glued-to-digits", "12x,13"), ("nul-byte", "1,\x00,3"), ("quote", '1,"2",3'), ("vertical-tab", "1,\x0b2"),
                        ("form-feed", "1,\x0c2"), ("byte-0xa0", b"1,\xa02")):
        yield _case(f"sep-{label}", mins_doc(body))
    around = [KM - 150 + i for i in range(300)]                               # json.dumps(..., indent=2) of a sketch: a value a line
    yield _case("sep-indent-2-form-300-values-around-keep-max", mins_doc("\n" + ",\n".join(" " * 10 + str(v) for v in around) + "\n" + " " * 8))
    # white-space runs behind a comma: in the middle of a chunk (comma at byte 2000) and at the chunk's last comma (byte 4095)
    for where, at in (("mid-chunk", 2000), ("chunk-last-comma", 4095)):
        for run in (62, 63, 64, 65):
            body = ",".join(tokens_of_len(at, maxd=18)) + "," + " " * run + str(10 ** 18 + 1) + "," + str(U64)
            yield _case(f"sep-white-space-run-{run}-behind-comma-{where}", mins_doc(body), may_fall_back=True)
        for stretch in (62, 63, 64, 65):                                      # white space + 19 digits = the stretch
            body = ",".join(tokens_of_len(at, maxd=18)) + "," + "\n" * (stretch - 19) + str(10 ** 18 + 1) + "," + str(U64)
            yield _case(f"sep-stretch-{stretch}-behind-comma-{where}", mins_doc(body), may_fall_back=stretch > 63)
    for stretch in (62, 63, 64, 65):                                          # in front of the first value / behind the last
        yield _case(f"sep-stretch-{stretch}-first-value", mins_doc(" " * (stretch - 2) + "17,18"), may_fall_back=stretch > 63)
        yield _case(f"sep-stretch-{stretch}-last-value", mins_doc("17,18" + " " * (stretch - 2)), may_fall_back=stretch > 63)
    yield _case("sep-5000-bytes-of-white-space-in-front-of-the-first-value", mins_doc(" " * 5000 + "1,2"), may_fall_back=True)
    yield _case("sep-5000-bytes-of-white-space-and-nothing-else", mins_doc(" " * 5000), may_fall_back=True)


def _spans():
    yield _case("span-close-at-tile-bit-0-of-the-second-tile", mins_doc(body_of_len(64), back=b'],"x":1}'))
    yield _case("span-close-at-tile-bit-63", mins_doc(body_of_len(63), back=b'],"x":1}'))
    yield _case("span-close-at-tile-bit-0-of-the-first-tile-then-digits", mins_doc(b"", back=b'],"x":[1,2,3]}'))
    yield _case("span-commas-and-digits-behind-the-close-in-its-tile", mins_doc(b"1,2", back=b'],"x":[3,4,5,6],"y":7,"z":"a,b,c"}'))
    yield _case("span-odd-bytes-behind-the-close-in-its-tile", mins_doc(b"1,2", back=b'],"name":"x-y.z"}'))
    yield _case("span-second-array-in-the-tile-of-the-first-close", b'{"mins":[1,2],"abundances":[3,4]}')
    for at in range(58, 66):
        yield _case(f"span-key-begins-at-byte-{at}-of-the-key-search-tile", b'{"n":"' + b"x" * (at - 8) + b'",' + b'"mins":[1,2,3]}')
        yield _case(f"span-abundances-key-begins-at-byte-{at}", b'{"mins":[1],"n":"' + b"x" * (at - 8) + b'",' + b'"abundances":[7]}')
    for label, tail, fix in (("key", b'"mins"', b":0}"), ("key-colon", b'"mins":', b"0}"), ("key-colon-bracket", b'"mins":[', b""),
                             ("key-spaces-colon-bracket", b'"mins" : [', b""), ("key-colon-bracket-digit", b'"mins":[1', b""),
                             ("half-a-key", b'"min', b'":0}'), ("abundances-key", b'"abundances"', b":0}")):
        yield _case(f"span-document-ends-with-{label}", b'{"a":1,' + tail, json_fix=fix)
    yield _case("span-mins-is-an-object", b'{"mins":{"a":[1,2]}}')
    yield _case("span-abundances-null", b'{"mins":[1,2],"abundances":null}')
    yield _case("span-xmins", b'{"xmins":[1,2]}')
    yield _case("span-minsx", b'{"minsx":[1,2]}')
    yield _case("span-mins-as-a-string-value", b'{"name":"mins","mins":[4,5]}')
    yield _case("span-white-space-around-the-colon", b'{"mins" \n\r\t: \n\r\t[1,2]}')
    yield _case("span-8-arrays", b"[" + b",".join(b'{"mins":[%d,%d]}' % (i, i + 100) for i in range(8)) + b"]")
    yield _case("span-9-arrays", b"[" + b",".join(b'{"mins":[%d,%d]}' % (i, i + 100) for i in range(9)) + b"]")
    yield _case("span-mins-and-abundances-alternating-8", b"[" + b",".join(b'{"mins":[%d,%d],"abundances":[9,9]}' % (i, i + 100) for i in range(4)) + b"]")
    yield _case("span-mins-and-abundances-alternating-9-th-is-mins", b"[" + b",".join(b'{"mins":[%d,%d],"abundances":[9,9]}' % (i, i + 100) for i in range(5)) + b"]")
    yield _case("span-abundances-with-a-float", b'{"mins":[1,2],"abundances":[1.5,2]}')
    yield _case("span-no-array", b'{"class":"sourmash_signature","version":0.4}')
    yield _case("span-document-of-1-byte", b"{", json_fix=b"}")
    yield _case("span-document-of-1-byte-a-quote", b'"', json_fix=b'"')
    yield _case("span-no-closing-bracket-next-document-begins-with-digits", b'{"mins":[1,2', behind=b'3,4],"mins":[5,6]}')
    yield _case("span-second-array-has-no-closing-bracket", b'{"mins":[1,2],"mins":[3,4', behind=b"]]]]")


DEFECTS = ("equal", "descending", "2^64", "21-digits", "letter", "dot", "minus", "double-comma", "trailing-comma", "space-for-comma", "missing-first")


def _random():
    """300 seeded arrays: 0 .. 3 chunks long, values of 1 .. 20 digits, white space behind a separator with probability 0.2 -- 1 .. 40
    bytes, one run in a thousand 41 .. 70 (which keeps the share of arrays with a stretch above 63 bytes under one in ten) -- and a
    defect planted in every fourth"""
    rng = np.random.default_rng(20240)
    for r in range(300):
        target = int(rng.integers(0, 3 * CHUNK + 1))
        vals, size = set(), 0
        while size < target:
            d = int(rng.integers(1, 21))
            v = int(rng.integers(10 ** (d - 1), 10 ** d, dtype=np.uint64)) if d < 20 else 10 ** 19 + int(rng.integers(0, 8 * 10 ** 18))
            if v not in vals:
                vals.add(v)
                size += d + 1
        toks = [str(v) for v in sorted(vals)] if target else []
        defect = DEFECTS[(r // 4) % len(DEFECTS)] if r % 4 == 0 and len(toks) >= 3 else None
        j = int(rng.integers(0, max(1, len(toks) - 1)))
        if defect == "equal":
            toks[j + 1] = toks[j]
        elif defect == "descending":
            toks[j], toks[j + 1] = toks[j + 1], toks[j]
        elif defect == "2^64":
            toks[-1] = str(2 ** 64 + int(rng.integers(0, 1000)))
        elif defect == "21-digits":
            toks[-1] = str(10 ** 20 + 3)
        elif defect == "letter":
            toks[j] += "e"
        elif defect == "dot":
            toks[j] += ".0"
        elif defect == "minus":
            toks[j] = "-" + toks[j]
        elif defect == "double-comma":
            toks[j] += ","
        elif defect == "trailing-comma":
            toks[-1] += ","
        elif defect == "space-for-comma":
            toks[j] = toks[j] + " " + toks.pop(j + 1)
        elif defect == "missing-first":
            toks[0] = ""
        parts = []
        for i, t in enumerate(toks):
            run = 0
            if rng.random() < 0.2:
                run = int(rng.integers(41, 71)) if rng.random() < 0.001 else int(rng.integers(1, 41))
            parts.append(bytes(rng.choice(np.frombuffer(b" \n\r\t", dtype=np.uint8), size=run)) + t.encode())
        body = b",".join(parts)
        name = f"random-{r:03d}" + (f"-{defect}" if defect else "")
        yield _case(name, mins_doc(body), may_fall_back=defect is None and longest_stretch(body) > AHEAD - 1 and ref_array(body, KM)[0])


@functools.lru_cache(maxsize=None)
def named_cases():
    "every case that is not random"
    out = []
    for gen in (_sizes, _sweeps, _look_ahead, _alignment, _limit, _order, _separators, _spans, _end_of_block):
        out.extend(gen())
    return tuple(out)


@functools.lru_cache(maxsize=None)
def random_cases():
    return tuple(_random())


def all_cases():
    return named_cases() + random_cases()


@functools.lru_cache(maxsize=None)
def by_name():
    d = {c.name: c for c in all_cases()}
    assert len(d) == len(all_cases()), "two cases share a name"
    return d


# ---- text blocks ------------------------------------------------------------------------------------------------------------------
Block = namedtuple("Block", "name keep_max text docs cases")       # docs: [(off, len)] of cases[i]


def _layout(name, keep_max, cases):
    """documents side by side, each moved (by filler that is itself digits, commas and brackets) to where the first byte of its
    first array -- or of the document, if it has none -- has the address case.align modulo 16 in a block that begins on a line"""
    text, docs = bytearray(), []
    for c in cases:
        spans, _ = ref_spans(c.doc)
        first = spans[0].begin if spans else 0
        fill = (c.align - (len(text) + first)) % 16
        text += (b"7,]" * 6)[:fill]
        docs.append((len(text), len(c.doc)))
        text += c.doc + c.behind
    return Block(name, keep_max, bytes(text), tuple(docs), tuple(cases))


@functools.lru_cache(maxsize=None)
def blocks():
    """the cases in a handful of text blocks: one per keep_max for the named cases and for the random ones, and every end-of-block
    case as the last document of a small block of its own (a few cases in front of it)"""
    out = []
    for label, cases in (("named", named_cases()), ("random", random_cases())):
        for km in sorted({c.keep_max for c in cases}):
            some = [c for c in cases if c.keep_max == km and not c.last]
            if some:
                out.append(_layout(f"{label}-keep-max-{km}", km, some))
    front = [c for c in named_cases() if c.name.startswith("size-6")]
    for c in named_cases():
        if c.last:
            out.append(_layout(c.name, c.keep_max, front + [c]))
            assert out[-1].docs[-1][0] + out[-1].docs[-1][1] == len(out[-1].text)
    return tuple(out)


def plan(docs, spans, flags):
    """the jobs of the parse step from the span records of a block, as sigload.hpp plans them: a document with the odd bit or an
    odd array gives none, every `mins` array of the others one, their values side by side -> (JOB array, [(doc, span)] per job)"""
    jobs, where, n_values = [], [], 0
    for d, (off, _) in enumerate(docs):
        ns = int(flags[d]) & 0xff
        if int(flags[d]) & DOC_ODD or any(int(spans[d * MAX_SPANS + s]["flags"]) & 1 for s in range(ns)):
            continue
        for s in range(ns):
            sp = spans[d * MAX_SPANS + s]
            if int(sp["kind"]) == MINS:
                jobs.append((off + int(sp["begin"]), int(sp["end"]) - int(sp["begin"]), n_values, int(sp["n_values"])))
                where.append((d, s))
                n_values += int(sp["n_values"])
    return np.array(jobs, dtype=JOB), where, n_values


def check_doc(block, d, spans, flags, jobs, job_of, values, parsed, what):
    "the contract on document d of a block -> whether the parser took it and flagged none of its arrays"
    case = block.cases[d]
    exp = expected(case.name)
    ns = int(flags[d]) & 0xff
    got_spans = [RefSpan(int(sp["begin"]), int(sp["end"]), int(sp["kind"]), int(sp["n_values"]), bool(int(sp["flags"]) & 1))
                 for sp in spans[d * MAX_SPANS:d * MAX_SPANS + ns]]
    assert got_spans == exp.spans and bool(int(flags[d]) & DOC_ODD) == exp.doc_odd, (what, case.name, got_spans, exp.spans, hex(int(flags[d])))   # (c)
    assert int(flags[d]) & ~(DOC_ODD | 0xff) == 0, (what, case.name)
    doc_taken = not exp.doc_odd and not any(s.odd for s in exp.spans)
    mins = [s for s, sp in enumerate(exp.spans) if sp.kind == MINS]
    assert all(((d, s) in job_of) == doc_taken for s in mins), (what, case.name)
    if not doc_taken:
        return False
    clean = True
    for a, s in zip(exp.arrays, mins):
        j = job_of[(d, s)]
        flagged = bool(int(parsed[j]["flags"]) & 1)
        assert int(parsed[j]["flags"]) & ~1 == 0, (what, case.name)
        if not flagged:                                                                            # (a)
            lo = int(jobs[j]["value_off"])
            got = [int(v) for v in values[lo:lo + int(jobs[j]["n_values"])]]
            assert a.plain, (what, case.name, "an array that is not plain was not flagged", got[:8])
            assert got == a.values, (what, case.name, "values differ", [(i, g, w) for i, (g, w) in enumerate(zip(got, a.values)) if g != w][:4], len(got), len(a.values))
            assert int(parsed[j]["n_kept"]) == a.n_kept, (what, case.name, "n_kept", int(parsed[j]["n_kept"]), a.n_kept)
        elif a.plain and not a.long_stretch:                                                       # (b)
            raise AssertionError((what, case.name, "a plain array with stretches of at most 63 bytes was flagged"))
        clean = clean and not flagged
    return clean


def check_block(block, spans, flags, jobs, where, values, parsed, what):
    """the contract (a), (b), (c) of the module's docstring on what a parser -- the emulation or the device -- made of a block.
    -> the names of the cases whose documents it took and whose arrays it did not flag"""
    job_of = {w: j for j, w in enumerate(where)}
    return [block.cases[d].name for d in range(len(block.cases)) if check_doc(block, d, spans, flags, jobs, job_of, values, parsed, what)]


# ---- whole signatures for the loader ----------------------------------------------------------------------------------------------
def array_body(name, which=0):
    "the bytes of a named case's `which`-th `mins` array"
    case = by_name()[name]
    sp = [s for s in ref_spans(case.doc)[0] if s.kind == MINS][which]
    return case.doc[sp.begin:sp.end]
