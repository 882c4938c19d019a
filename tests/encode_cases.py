"""Edge cases for the Snappy block encoder (device: csrc/rio_encode.hip, host: rio_writer.cpp, checker:
oracle/rio_oracle.c) and a parser that says which encoder branches a stream went through.

`elements` walks a Snappy block stream and asserts what holds for anything golang/snappy v1.0.0 emits
(encode.go, encode_other.go): these follow from the format and from emitCopy's rule, not from any of
the three restatements. `classes` turns the elements into labels; every case family declares the
labels it must produce, so a family cannot silently stop covering its branch
(tests/test_encode_cases.py checks that on the CPU, tests/test_gpu_encode_edges.py runs the device).

Labels:
  lit1=N lit2=N lit3=N   a literal of N bytes with a 1-, 2- or 3-byte tag
  c1=N                   a tag-01 copy (2 bytes) of length N
  far=N                  a tag-10 copy of length N <= 11 that is not a chain's end (so offset >= 2048)
  copy=N                 a logical copy (maximal run of adjacent copy elements with one offset) of N bytes
  split=A+B+..           the element lengths of a logical copy of more than one element
  overlap                a copy whose offset is smaller than its length
  copy@>P                a copy element that starts above position P of its 64 KiB block (P = 32768, 65000)
  tail[b]=N              block b ends in a literal of N bytes (0: it ends in a copy)
  blocks=K               the stream has K 64 KiB blocks
"""
import ctypes
import random

import numpy as np

import oracle_py as orc

BLOCK = 65536


def uvarint(buf, i=0):
    v = s = 0
    while True:
        c = buf[i]
        i += 1
        v |= (c & 0x7F) << s
        s += 7
        if c < 0x80:
            return v, i


def elements(stream):
    """[(class, length, offset, position)] of a Snappy block stream; class is "lit1", "lit2", "lit3",
    "c1" (tag 01) or "c2" (tag 10), offset 0 for literals, position the element's first output byte."""
    total, i = uvarint(stream)
    out, pos = [], 0
    while i < len(stream):
        tag = stream[i]
        kind = tag & 3
        if kind == 0:
            m = tag >> 2
            assert m < 62, f"literal with a {m - 59}-byte length field at {i}"
            if m < 60:
                cls, ln, i = "lit1", m + 1, i + 1
            elif m == 60:
                cls, ln, i = "lit2", stream[i + 1] + 1, i + 2
            else:
                cls, ln, i = "lit3", (stream[i + 1] | stream[i + 2] << 8) + 1, i + 3
            off = 0
            i += ln
            assert i <= len(stream), "literal runs past the stream"
        elif kind == 1:
            cls, ln, off = "c1", 4 + (tag >> 2 & 7), (tag >> 5) << 8 | stream[i + 1]
            i += 2
            assert 4 <= ln <= 11 and off < 2048
        elif kind == 2:
            cls, ln, off = "c2", 1 + (tag >> 2), stream[i + 1] | stream[i + 2] << 8
            i += 3
            if not (ln >= 12 or off >= 2048):  # only as the end of an emitCopy chain
                p = out[-1] if out else None
                assert p and p[0] == "c2" and p[1] in (64, 60) and p[2] == off and p[3] + p[1] == pos, (
                    f"tag-10 copy of {ln} at offset {off} outside a chain (output position {pos})")
        else:
            raise AssertionError(f"4-byte-offset copy at {i}")
        if kind:  # blocks are encoded on their own: a copy reaches back inside its block only
            assert 0 < off <= pos % BLOCK, f"copy offset {off} at block position {pos % BLOCK}"
        assert pos // BLOCK == (pos + ln - 1) // BLOCK, f"element at {pos} of {ln} crosses a block"
        out.append((cls, ln, off, pos))
        pos += ln
    assert i == len(stream), "stream not consumed exactly"
    assert pos == total, f"elements sum to {pos}, preamble says {total}"
    return out


def split_copy(length):
    """emitCopy's pieces for one match (encode_other.go emitCopy)."""
    out = []
    while length >= 68:
        out.append(64)
        length -= 64
    if length > 64:
        out.append(60)
        length -= 60
    out.append(length)
    return out


def logical_copies(els):
    """[(offset, position, [element lengths])]: maximal runs of adjacent copy elements with one offset."""
    runs = []
    for cls, ln, off, pos in els:
        if cls[0] != "c":
            continue
        if runs and runs[-1][0] == off and runs[-1][1] + sum(runs[-1][2]) == pos and pos % BLOCK:
            runs[-1][2].append(ln)
        else:
            runs.append((off, pos, [ln]))
    return runs


def classes(stream):
    """The labels (module docstring) of one stream; asserts emitCopy's split on every logical copy."""
    els = elements(stream)
    lab = set()
    tails = {}
    for cls, ln, off, pos in els:
        b = pos // BLOCK
        if cls[0] == "l":
            lab.add(f"{cls}={ln}")
            tails[b] = ln
        else:
            tails[b] = 0
            if cls == "c1":
                lab.add(f"c1={ln}")
            elif ln <= 11 and off >= 2048:
                lab.add(f"far={ln}")
            if off < ln:
                lab.add("overlap")
            for p in (32768, 65000):
                if pos % BLOCK > p:
                    lab.add(f"copy@>{p}")
    for off, pos, pieces in logical_copies(els):
        n = sum(pieces)
        assert pieces == split_copy(n), f"copy of {n} at {pos} split as {pieces}, emitCopy gives {split_copy(n)}"
        lab.add(f"copy={n}")
        if len(pieces) > 1:
            lab.add("split=" + "+".join(map(str, pieces)))
    for b, t in tails.items():
        lab.add(f"tail[{b}]={t}")
    lab.add(f"blocks={len(tails)}")
    return lab


# ------------------------------------------------------------------------------------------------
# batches as arrays, the oracle on them, and per-record payloads of a file image
# ------------------------------------------------------------------------------------------------
def to_arrays(records):
    """(blob uint8, rec_off uint64 [n + 1], flags uint8 [n]) of a list of bytes / None (nil)."""
    n = len(records)
    off = np.zeros(n + 1, dtype=np.uint64)
    if n:
        np.cumsum([0 if r is None else len(r) for r in records], out=off[1:])
    blob = np.frombuffer(b"".join(r or b"" for r in records), dtype=np.uint8)
    flags = np.fromiter((r is None for r in records), dtype=np.uint8, count=n)
    return blob, off, flags


def oracle_arrays(blob, off, flags, comp):
    """orc_encode_file on arrays: (file image uint8, record offsets uint64 [n])."""
    n = int(off.shape[0]) - 1
    blob = np.ascontiguousarray(np.concatenate([blob, np.zeros(8, np.uint8)]))
    fl = np.ascontiguousarray(np.concatenate([flags, np.zeros(8, np.uint8)]).astype(np.uint8))
    total = int(off[-1] - off[0])
    cap = 8 + 72 * n + total + total // 6 + 64
    out = np.empty(cap, dtype=np.uint8)
    roff = np.zeros(max(n, 1), dtype=np.uint64)
    ln = orc.lib().orc_encode_file(blob.ctypes.data, off.ctypes.data, fl.ctypes.data, n, comp, out.ctypes.data, cap,
                                   roff.ctypes.data)
    assert ln
    return out[:ln], roff[:n]


def oracle_snappy(data):
    src = ctypes.create_string_buffer(bytes(data), len(data) + 1)
    dst = ctypes.create_string_buffer(32 + len(data) + len(data) // 6)
    k = orc.lib().orc_snappy_encode(dst, src, len(data))
    return dst.raw[:k]


def payloads(image, offs):
    """Per record of a v4 file image: (nil, u, c, payload bytes), from the headers at `offs`."""
    image = bytes(image)
    out = []
    ends = [int(o) for o in offs[1:]] + [len(image)]
    for o, end in zip((int(o) for o in offs), ends):
        assert image[o:o + 3] == b"\x91\x8d\x4c", f"no record magic at {o}"
        nil = image[o + 3]
        u, i = uvarint(image, o + 4)
        c, i = uvarint(image, i)
        _, i = uvarint(image, i)
        out.append((nil, u, c, image[i:end]))
    return out


# ------------------------------------------------------------------------------------------------
# the families
# ------------------------------------------------------------------------------------------------
def rnd(rng, n):
    return rng.randbytes(n)


def vocabulary(seed=7, words=400):
    rng = random.Random(seed)
    return [rnd(rng, rng.randint(3, 14)) for _ in range(words)]


def text(n, seed, vocab=None):
    """n bytes of words drawn from a vocabulary: matches of every short length at every distance."""
    rng = random.Random(seed)
    vocab = vocab or vocabulary()
    parts, have = [], 0
    while have < n:
        w = rng.choice(vocab)
        parts.append(w)
        have += len(w)
    return b"".join(parts)[:n]


class Family:
    """records: bytes / None; classes: labels some record's stream must carry; per_record: index ->
    labels that record's own stream must carry."""

    def __init__(self, name, records, classes_=(), per_record=None):
        self.name, self.records, self.classes = name, records, set(classes_)
        self.per_record = per_record or {}


COPY_LENGTHS = list(range(4, 14)) + list(range(59, 74)) + list(range(123, 134))


def fam_copy_lengths():
    recs = []
    for target in COPY_LENGTHS:
        for pre in (16, 17, 18, 19):  # both parities: after 32 probes the skip rule steps by 2
            for seed in range(3):
                rng = random.Random(target * 1000 + pre * 10 + seed)
                p = rnd(rng, target)
                recs.append(rnd(rng, pre) + p + rnd(rng, 20) + p + rnd(rng, 40))
    want = {f"copy={t}" for t in COPY_LENGTHS}
    want |= {"split=60+5", "split=60+6", "split=60+7", "split=64+4", "split=64+5", "split=64+60", "split=64+64+4"}
    return Family("copy_lengths", recs, want)


def fam_tag01_far():
    recs = [text(6000, 1), text(70000, 2)]
    want = {f"c1={n}" for n in range(4, 12)} | {f"far={n}" for n in range(4, 12)}
    return Family("tag01_far", recs, want)


LITERAL_SIZES = [16, 17, 18, 59, 60, 61, 62, 255, 256, 257, 258, 65535, 65536, 65537, 65536 + 16, 65536 + 17]


def fam_literals():
    rng = random.Random(31)
    recs = [rnd(rng, n) for n in LITERAL_SIZES]
    per = {LITERAL_SIZES.index(16): {"lit1=16"}, LITERAL_SIZES.index(17): {"lit1=17"},
           LITERAL_SIZES.index(60): {"lit1=60"}, LITERAL_SIZES.index(61): {"lit2=61"},
           LITERAL_SIZES.index(256): {"lit2=256"}, LITERAL_SIZES.index(257): {"lit3=257"},
           LITERAL_SIZES.index(65536): {"lit3=65536", "blocks=1"},
           LITERAL_SIZES.index(65537): {"lit3=65536", "lit1=1", "blocks=2"},
           LITERAL_SIZES.index(65536 + 16): {"lit3=65536", "lit1=16"},
           LITERAL_SIZES.index(65536 + 17): {"lit3=65536", "lit1=17"}}
    return Family("literals", recs, (), per)


TABLE_SIZES = [256 << k for k in range(7)]  # 256 .. 16384: the hash shift changes above each


def fam_table_sizes():
    base = text(BLOCK, 3)
    recs, per = [], {}
    for n in TABLE_SIZES:
        for m in (n, n + 1):
            per[len(recs)] = {"blocks=1"}
            recs.append(base[7:7 + m])
    # 131072 + 40 bytes, the table reset between blocks: the second block repeats the first, so every
    # entry the first one left behind would be a "match" at distance 0
    per[len(recs)] = {"blocks=3", "lit1=40"}
    recs.append(base + base + base[:40])
    return Family("table_sizes", recs, {"c1=4", "copy=12"}, per)


BLOCK_TAILS = [0, 1, 7, 14, 15, 16]


def fam_block_ends():
    recs, per = [], {}
    for k in BLOCK_TAILS:
        rng = random.Random(50 + k)
        p = rnd(rng, 40)
        per[len(recs)] = {f"tail[0]={k}", "blocks=1"}
        recs.append(rnd(rng, 18) + p + rnd(rng, 20) + p + rnd(rng, k))
    for k in BLOCK_TAILS:  # the same shape ending exactly at byte 65536 of a 70000-byte record
        rng = random.Random(70 + k)
        p = rnd(rng, 40)
        end = p + rnd(rng, 20) + p + rnd(rng, k)
        per[len(recs)] = {f"tail[0]={k}", "blocks=2"}
        recs.append(text(BLOCK - len(end), 60 + k) + end + text(70000 - BLOCK, 80 + k))
        assert len(recs[-1]) == 70000
    return Family("block_ends", recs, (), per)


def fam_high_positions():
    # a prefix that keeps matching (a long random prefix lets the skip rule step over the match)
    return Family("high_positions", [text(BLOCK, 4)], (), {0: {"copy@>32768", "copy@>65000", "blocks=1"}})


RUN_SIZES = [17, 100, 1024, 1025, 150000]


def fam_runs():
    recs = []
    for n in RUN_SIZES:
        recs.append(bytes(n))
        for period in (1, 2, 3, 7):
            unit = bytes(range(0x41, 0x41 + period))
            recs.append((unit * (n // period + 1))[:n])
    # a whole block as one chain: 1 literal byte, then 65535 = 1023 * 64 + 63; 7 literal bytes, then 65529
    return Family("runs", recs, {"overlap", "blocks=3", "copy=65535", "copy=65529", "copy=18927", "copy=16", "copy=99",
                                  "copy=93", "copy=1024"})


def fam_skip():
    rng = random.Random(90)
    a, b = rnd(rng, 5000), text(3000, 5, vocabulary(11, 100))
    # after 5000 bytes without a match the probes are about 160 bytes apart and step over the text
    # too: one literal; the other way round the text compresses and the random tail is one literal
    return Family("skip_rule", [a + b, b + a], (), {0: {"lit3=8000"}, 1: {"tail[0]=5000", "c1=4", "copy=12"}})


def fam_nil_empty():
    x, y = b"xyz", text(300, 6)
    recs = [None, b"", x, None, None, None, y, b"", b"", b"", x, None, b"", None, b"", y, b"", None]
    more = [[None], [b""], [b"", x, None], [None, x, b""], [x, y, None], [x, y, b""]]
    return Family("nil_empty", recs + [r for batch in more for r in batch], {"lit1=3", "blocks=1"})


def families():
    return [fam_copy_lengths(), fam_tag01_far(), fam_literals(), fam_table_sizes(), fam_block_ends(),
            fam_high_positions(), fam_runs(), fam_skip(), fam_nil_empty()]


_FAMILIES = None


def cached_families():
    """families(), built once per process; nobody changes them."""
    global _FAMILIES
    if _FAMILIES is None:
        _FAMILIES = families()
    return _FAMILIES


def nil_span_batch():
    """Raw arrays with one nil record whose arena span is not empty (flag set, rec_off[i+1] >
    rec_off[i]) and the list it must encode like: the span is skipped, u = 0."""
    a, hidden, b = text(200, 8), text(90, 9), text(1500, 10)
    blob = np.frombuffer(a + hidden + b, dtype=np.uint8)
    off = np.array([0, 200, 290, 1790], dtype=np.uint64)
    flags = np.array([0, 1, 0], dtype=np.uint8)
    return (blob, off, flags), [a, None, b]


def shuffled_all(seed=1234):
    """Every family's records in one batch, in a seeded shuffled order: [(family, index, record)]."""
    items = [(f.name, i, r) for f in cached_families() for i, r in enumerate(f.records)]
    random.Random(seed).shuffle(items)
    return items


def launch_global_reuse():
    """8192 + 64 + 1 records of 1025..1100 bytes of text with a 70000-byte record below index 8192
    and one above: with 8192 global table slots, a slot is reused across different table sizes."""
    n = 8192 + 64 + 1
    rng = np.random.default_rng(5)
    pool = text(1 << 20, 11)
    lens = rng.integers(1025, 1101, n)
    starts = rng.integers(0, len(pool) - 1200, n)
    recs = [pool[int(s):int(s) + int(k)] for s, k in zip(starts, lens)]
    recs[10] = text(70000, 12)
    # the same lane and slot as record 10 with the default 128 groups, and the same bytes: every entry
    # record 10 left behind would be a "match" at distance 0
    recs[10 + 8192] = recs[10]
    recs[8192 + 37] = text(70000, 14)
    return to_arrays(recs)


def launch_lds_second_pass():
    """262144 + 16 + 1 records of 17..40 compressible bytes (three symbols)."""
    n = 262144 + 16 + 1
    rng = np.random.default_rng(6)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(rng.integers(17, 41, n), out=off[1:])
    blob = rng.integers(0x61, 0x64, int(off[-1]), dtype=np.uint8)
    return blob, off, np.zeros(n, dtype=np.uint8)


def launch_million_tiny():
    """1048576 + 300 records of 0..3 bytes, some nil."""
    n = 1048576 + 300
    rng = np.random.default_rng(7)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(rng.integers(0, 4, n), out=off[1:])
    blob = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    flags = (rng.integers(0, 16, n) == 0).astype(np.uint8)
    return blob, off, flags
