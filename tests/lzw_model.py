"""Go's compress/lzw reader (LSB, litWidth 8) restated, a code-stream writer with the reader's width
schedule, and crafted streams the reference's writer never emits.

The writer of the reference clears its table at 3838 codes, so nothing it produces reaches the region
the device decoder (csrc/rio_lzw.hip) leans on: Go's reader keeps decoding with a full table (width
12: no new entries, `last` invalid, hi stays 4095, code 4095 a plain lookup), and the kernel's
closed-form width / bit position, its `hi = min(257 + k, 4095)` and its 3840-entry table have to agree
with that for as long as the epoch lasts. `decode` is the independent statement of the reader (beside
the oracle's C restatement); `cases` builds the streams from code lists.
"""
import functools
import random

import corpus

CORRUPT = "corrupt"
CLEAR, EOF, INVALID = 256, 257, 0xFFFF



def decode(data):
    """bytes, or CORRUPT ("lzw: invalid code" / io.ErrUnexpectedEOF), of one payload."""
    bits = nbits = ip = 0
    width, hi, overflow, last = 9, EOF, 1 << 9, INVALID
    prefix, suffix = [0] * 8192, [0] * 8192
    out = bytearray()
    while True:
        while nbits < width:
            if ip >= len(data):
                return CORRUPT
            bits |= data[ip] << nbits
            ip += 1
            nbits += 8
        code = bits & ((1 << width) - 1)
        bits >>= width
        nbits -= width
        if code < CLEAR:
            out.append(code)
            if last != INVALID:
                suffix[hi], prefix[hi] = code, last
        elif code == CLEAR:
            width, hi, overflow, last = 9, EOF, 1 << 9, INVALID
            continue
        elif code == EOF:
            return bytes(out)
        elif code <= hi:
            c, tail = code, bytearray()
            if code == hi and last != INVALID:  # KwKwK: last's expansion followed by its own first byte
                c = last
                while c >= CLEAR:
                    c = prefix[c]
                tail.append(c)
                c = last
            while c >= CLEAR:
                tail.append(suffix[c])
                c = prefix[c]
            tail.append(c)
            out += tail[::-1]
            if last != INVALID:
                suffix[hi], prefix[hi] = c, last
        else:
            return CORRUPT
        last, hi = code, hi + 1
        if hi >= overflow:
            if width == 12:  # table full: nothing is added until a clear, and hi stays 4095 (`r.hi--`)
                last = INVALID
                hi -= 1
            else:
                width += 1
                overflow = 1 << width


def width_of(k):
    """Width of code k of an epoch (k counts from the last clear): 9 bits for 0..254, 10 to 766, 11 to 1790."""
    return 9 if k < 255 else 10 if k < 767 else 11 if k < 1791 else 12


def pack(codes):
    """The LSB-first byte stream of a code list under the reader's width schedule."""
    bits = nb = k = 0
    out = bytearray()
    for c in codes:
        w = width_of(k)
        assert c < 1 << w, (c, k)
        bits |= c << nb
        nb += w
        while nb >= 8:
            out.append(bits & 0xFF)
            bits >>= 8
            nb -= 8
        k = 0 if c == CLEAR else k + 1
    if nb:
        out.append(bits & 0xFF)
    return bytes(out)


def random_codes(rng, n, k=0, kwkwk=0.1):
    """n valid codes continuing an epoch at index k: literals, defined entries, code == hi."""
    out = []
    for _ in range(n):
        top = min(257 + k, 4095)  # hi before code k; entries 258 .. top - 1 are defined, top is KwKwK
        full = k > 3838
        r = rng.random()
        if k == 0 or r < 0.3 or top < 259:
            c = rng.randrange(256)
        elif r < 0.3 + kwkwk and not full:
            c = top
        else:
            c = rng.randint(258, top if full else top - 1)
        out.append(c)
        k += 1
    return out


def literals(rng, n):
    return [rng.randrange(256) for _ in range(n)]


def cases():
    """[(name, payload)]: the model says what each decodes to."""
    rng = random.Random(4095)
    out = []
    full = lambda: literals(rng, 3838)  # noqa: E731  codes 0..3837 of an epoch: entries 258..4094
    tail = [300, 4095, 65, 4000, 258, 4094, 4093, 259]
    # the table fills at code 3838 (it defines entry 4095); from 3839 on nothing is added
    out.append(("full_4094_then_4095", pack([CLEAR] + full() + [4094, 4095, 4095] + tail +
                                            [rng.randint(258, 4095) for _ in range(500)] + [EOF])))
    out.append(("full_kwkwk_at_3838", pack([CLEAR] + full() + [4095, 4095, 4095] + tail +
                                           [rng.randint(258, 4095) for _ in range(500)] + [EOF])))
    out.append(("full_no_leading_clear", pack(full() + [4095, 4095, 300, 4094] + [EOF])))
    out.append(("full_literal_at_3838", pack([CLEAR] + full() + [7, 4095, 4095, 4094] + tail + [EOF])))
    # a shorter epoch before the clear: the decoder's rounds of 64 codes restart at every clear, so code
    # 3838 of an epoch is lane 62 of its round wherever the epoch starts in the stream
    out.append(("full_after_63", pack([CLEAR] + random_codes(rng, 63) + [CLEAR] + full() +
                                      [4095, 4095, 4095, 4094] + tail + [EOF])))
    # the epoch goes on for thousands of codes past the full table
    out.append(("full_then_6000", pack([CLEAR] + random_codes(rng, 3838) + random_codes(rng, 6000, 3838) + [EOF])))
    out.append(("full_then_clear", pack([CLEAR] + random_codes(rng, 3900) + [CLEAR] + random_codes(rng, 700) +
                                        [CLEAR] + random_codes(rng, 5000) + [EOF])))
    out.append(("full_to_the_code", pack([CLEAR] + random_codes(rng, 3838) + [EOF])))
    out.append(("full_plus_one", pack([CLEAR] + random_codes(rng, 3839) + [EOF])))
    out.append(("full_plus_two", pack([CLEAR] + random_codes(rng, 3838) + [4095, 4095, EOF])))
    # invalid: 4095 before it is defined (12-bit codes from index 1791); hi + 1 at every width step
    out.append(("bad_4095_early", pack([CLEAR] + literals(rng, 1800) + [4095, EOF])))
    out.append(("bad_4095_at_3837", pack([CLEAR] + full()[:3837] + [4095, EOF])))
    for k in (255, 767, 1791):
        out.append((f"kwkwk_at_{k}", pack([CLEAR] + literals(rng, k) + [257 + k, 258, EOF])))
        out.append((f"bad_hi_plus_1_at_{k}", pack([CLEAR] + literals(rng, k) + [258 + k, EOF])))
        out.append((f"kwkwk_at_{k - 1}", pack([CLEAR] + literals(rng, k - 1) + [256 + k, 258, EOF])))
    out.append(("bad_hi_plus_1_at_1", pack([CLEAR, 65, 259, EOF])))
    out.append(("bad_copy_first", pack([CLEAR, 258, EOF])))
    # KwKwK chains: every code is the entry being defined (lengths 2, 3, 4, ..)
    for n in (64, 65, 130, 200):
        out.append((f"kwkwk_chain_{n}", pack([CLEAR, 120] + [258 + j for j in range(n)] + [65, 258 + n // 2, EOF])))
    out.append(("kwkwk_chain_offset", pack([CLEAR] + literals(rng, 37) + [257 + 37 + j for j in range(100)] + [EOF])))
    # copies around the 64-byte windows the output is written in: 64 literals (one round, bytes 0..63),
    # then entries that end at byte 64 (320), straddle it (321) and start there (322)
    lit64 = literals(rng, 64)
    out.append(("window_edges", pack([CLEAR] + lit64 + [320, 321, 322, 322, 321, 320, 323, 324] +
                                     random_codes(rng, 200, 72) + [EOF])))
    # 16-bit positions: 65535 decoded bytes from a payload the small class takes, and 65536 bytes from a
    # payload of the same size (the large class): a literal, 360 KwKwK codes (65341 bytes), one more entry
    chain = [CLEAR, 90] + [258 + j for j in range(360)]
    for want, last in ((65535, 257 + 193), (65536, 257 + 194), (65534, 257 + 192)):
        p = pack(chain + [last, EOF])
        out.append((f"decodes_to_{want}", p + bytes(1000 - len(p))))
    # payload sizes at the class boundary: codes up to the byte budget, eof, bytes after it ignored
    for size in (1151, 1152, 1153):
        codes = [CLEAR] + random_codes(rng, 900, kwkwk=0.02)
        while len(pack(codes + [EOF])) > size:
            codes.pop()
        p = pack(codes + [EOF])
        out.append((f"payload_{size}", p + b"\xa5" * (size - len(p))))
    for n in (200, 1500, 5000):
        out.append((f"random_codes_{n}", pack([CLEAR] + random_codes(rng, n) + [EOF])))
    return out


@functools.lru_cache(maxsize=None)
def case_items():
    """[(name, (u, payload), expected bytes or CORRUPT)]; u is the decoded length (10 where corrupt)."""
    out = []
    for name, p in cases():
        r = decode(p)
        out.append((name, (len(r) if r is not CORRUPT else 10, p), r))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def files():
    """[(name, lzw image, expected per record)]: the valid streams, then each invalid one between good
    records, then everything shuffled into one file."""
    items = case_items()
    good = [(n, it, r) for n, it, r in items if r is not CORRUPT]
    badc = [(n, it, r) for n, it, r in items if r is CORRUPT]
    out = [("lzw_edges_valid", corpus.lzw_file([it for _, it, _ in good]), [r for _, _, r in good])]
    mix, exp = [], []
    for k, (_, it, r) in enumerate(badc):
        for g in (good[(2 * k) % len(good)], None, good[(2 * k + 1) % len(good)]):
            mix.append(it if g is None else g[1])
            exp.append(r if g is None else g[2])
    out.append(("lzw_edges_refused", corpus.lzw_file(mix), exp))
    rng = random.Random(5)
    allc = list(items)
    rng.shuffle(allc)
    out.append(("lzw_edges_shuffled", corpus.lzw_file([it for _, it, _ in allc]), [r for _, _, r in allc]))
    return tuple(out)


FILE_NAMES = ("lzw_edges_valid", "lzw_edges_refused", "lzw_edges_shuffled")  # files()'s, without building them


def redo_file(n=2500, every=50, seed=8):
    """(image, records, indices whose header u is not the decoded length): text records through the
    oracle's writer; every `every`-th header claims 7 bytes more or fewer, so k_lzw_decode hands the
    record to k_lzw_resize and the redo round. Long enough for more than 1536 chunks of 256 bytes."""
    import oracle_py as orc

    recs = corpus.text_records(n, seed, 200, 400)
    redo = list(range(every - 1, n, every))
    items = [(len(r) + ((7 if (i // every) % 2 else -7) if i in set(redo) else 0), orc.lzw_encode(r))
             for i, r in enumerate(recs)]
    return corpus.lzw_file(items), recs, redo


def embedded_redo_file(n=60, every=10, seed=33):
    """(image, records, redo indices): every payload is followed, after its eof code, by the bytes of a
    recordio file (the reader ignores them), so chunk starts inside them find CRC-valid headers that are
    not on the chain and the placement comes from the sequential repair; every `every`-th header's u is
    off. k_lzw_resize documents a hand-back at the first such record for these files (`st->slow`)."""
    import oracle_py as orc

    inner = [bytes(r) for r in corpus.embedded_file_records(n, seed)]
    recs = corpus.text_records(n, seed, 50, 300)
    redo = list(range(every - 1, n, every))
    marked = set(redo)
    items = [(len(r) + (5 if i in marked else 0), orc.lzw_encode(r) + inner[i - i % 2]) for i, r in enumerate(recs)]
    return corpus.lzw_file(items), recs, redo
