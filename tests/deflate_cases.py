"""Hand-built DEFLATE / gzip records for the device inflate (csrc/rio_gzip.hip), and a tracer that says
which decoder branches a payload goes through.

zlib's compressor never emits most of what the kernel has code for: codes longer than 11 bits, one-bit
codes, distances at the window's edge, stored blocks at every bit misalignment, thousands of empty
blocks, headers Go accepts and zlib would not write. The builder here writes such streams bit by bit
from a token list and expands the tokens itself, so the expected bytes come from neither decoder.

`trace` is a small inflate of its own with Go's acceptance rules (compress/flate inflate.go,
huffmanDecoder.init; compress/gzip for the member framing): the independent reference beside the
oracle (whose DEFLATE is zlib's), and the self-check of the families: it returns labels for the
branches it met, and every family declares the labels it must produce
(tests/test_deflate_cases.py checks that on the CPU, tests/test_gpu_gzip_edges.py runs the device).

Labels:
  ll=N dl=N cl=N        a litlen / distance / code-length code of N bits was decoded
  r16xN r17xN r18xN     a repeat symbol with count N;  r16after17 r16after18: 16 repeating a zero run
  cross16 cross18       a run that starts in the litlen lengths and ends in the distance lengths
  end16 end17 end18     a run that ends exactly at HLIT + HDIST
  plain>64              more than 64 plain code lengths in a row
  cl1run>=130           a plain length with a one-bit code-length code, >= 130 times in a row
  lit1run>=300          >= 300 consecutive one-bit literal codes;  brkP: the symbol that ends such a run
                        starts at stream bit P mod 64 (the kernel's 64-offset lookup counts from where its bit
                        buffer stood, 33..64 bits per refill, not from the stream: the stream phase only spreads
                        the breaks over its offsets)
  mL@D                  a match of length L at distance D;  m258via284: length 258 as symbol 284 + 31
  dsSlo dsShi           distance symbol S with all-zero / all-one extra bits
  full@first full@break full@member   a match whose distance is all the member has produced: in its
                        first block, after a block break, in a later member
  d32768@>65536         distance 32768 at an output position past 65536
  srcx32768 dstx32768 srcx1024 dstx1024   a match whose source / destination straddles a multiple
  stN                   a stored block of LEN N;  statK: its header starts K bits into a byte
  st0final st0open      an empty stored block that is / is not the last
  blocksN               the record has N blocks;  types3: stored, fixed and dynamic blocks
  tokN                  the widest token (code + extra bits, both halves of a match) has N bits
  x1024 x128            a token straddles a multiple of 1024 / 128 bytes of the payload
  hlitN hdistN hclenN   dynamic header fields (as counts: 257.., 1.., 4..)
  one_dist_code empty_dist one_ll_code   Go's single one-bit code / empty distance code, accepted
  members=N             gzip members in the record
  refused: WHY          the rule the record was refused by
"""
import random
import struct
import zlib

import corpus

CORRUPT = "corrupt"
ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def _bases():
    lb, le = [], []
    for i in range(29):
        eb = 0 if i < 8 or i == 28 else (i - 4) >> 2
        lb.append(258 if i == 28 else (3 + i if i < 8 else ((4 + (i & 3)) << eb) + 3))
        le.append(eb)
    db, de = [], []
    for s in range(30):
        eb = 0 if s < 4 else (s - 2) >> 1
        db.append(s + 1 if s < 4 else ((2 + (s & 1)) << eb) + 1)
        de.append(eb)
    return lb, le, db, de


LBASE, LEXTRA, DBASE, DEXTRA = _bases()
assert LBASE[:9] == [3, 4, 5, 6, 7, 8, 9, 10, 11] and LBASE[27] == 227 and DBASE[29] == 24577 and DEXTRA[29] == 13


def len_sym(length, alt=False):
    """(symbol, extra bits, extra value); alt: 258 as symbol 284 with extra 31 (RFC 1951 allows both)."""
    if length == 258:
        return (284, 5, 31) if alt else (285, 0, 0)
    i = max(k for k in range(28) if LBASE[k] <= length)
    assert length - LBASE[i] < 1 << LEXTRA[i]
    return 257 + i, LEXTRA[i], length - LBASE[i]


def dist_sym(dist):
    s = max(k for k in range(30) if DBASE[k] <= dist)
    assert dist - DBASE[s] < 1 << DEXTRA[s]
    return s, DEXTRA[s], dist - DBASE[s]


# ---- writer ---------------------------------------------------------------------------------------
class Bits:
    """LSB-first bit writer; Huffman codes go in MSB-first (RFC 1951 3.1.1)."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        assert 0 <= v < 1 << n
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, cl):
        c, ln = cl
        self.put(int(format(c, f"0{ln}b")[::-1], 2), ln)

    def align(self):
        if self.n:
            self.out.append(self.acc)
            self.acc = self.n = 0

    def raw(self, b):
        assert self.n == 0
        self.out += b

    @property
    def phase(self):
        return self.n


def canonical(lengths):
    """{symbol: (code, length)} by RFC 1951 3.2.2. For an over-subscribed vector the codes wrap (such
    a table is only ever written, never used)."""
    cnt = [0] * 16
    for ln in lengths:
        cnt[ln] += 1
    cnt[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + cnt[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, ln in enumerate(lengths):
        if ln:
            out[s] = (nxt[ln] & ((1 << ln) - 1), ln)
            nxt[ln] += 1
    return out


def kraft(lengths):
    """Sum of 2^-len in units of 2^-15 (32768 = complete)."""
    return sum(1 << (15 - ln) for ln in lengths if ln)


def flat_lengths(used, size, rng):
    """A complete code over `used` (>= 2 symbols) with two adjacent lengths."""
    used = sorted(set(used))
    assert len(used) >= 2
    k = (len(used) - 1).bit_length()
    short = set(rng.sample(used, (1 << k) - len(used)))
    out = [0] * size
    for s in used:
        out[s] = k - 1 if s in short else k
    assert kraft(out) == 32768
    return out


def stair(top):
    """Lengths 1, 2, .., top, top + 1, top + 1: complete, every length up to top + 1 in use."""
    return list(range(1, top + 1)) + [top + 1, top + 1]


def shaped(symbols, shape, size, rng, pin=None):
    """`shape` (a complete multiset of lengths) dealt to `symbols` in a seeded order; pin: {symbol: length}."""
    assert len(symbols) == len(shape) and kraft(shape) == 32768
    shape, symbols = list(shape), list(symbols)
    out = [0] * size
    for s, ln in (pin or {}).items():
        shape.remove(ln)
        symbols.remove(s)
        out[s] = ln
    rng.shuffle(shape)
    for s, ln in zip(symbols, shape):
        out[s] = ln
    return out


class Blk:
    """Block break: the tokens after it go into a block of this kind. kind: "stored", "fixed", "dyn".
    dyn: ll / dl the litlen / distance length vectors (None: a flat code over the symbols the block
    uses), cl the 19 code-length code lengths (None: flat over what the header uses), rle the header
    as items (an int = that length plain, (16 | 17 | 18, count) a run; None: all plain), hlit / hdist /
    hclen raw field values where they should not follow from the vectors. stored: ln / nlen override
    LEN / NLEN. final: None = set on the record's last block."""

    def __init__(self, kind, final=None, ll=None, dl=None, cl=None, rle=None, hlit=None, hdist=None, hclen=None,
                 ln=None, nlen=None):
        self.kind, self.final, self.ll, self.dl, self.cl, self.rle = kind, final, ll, dl, cl, rle
        self.hlit, self.hdist, self.hclen, self.ln, self.nlen = hlit, hdist, hclen, ln, nlen


class Raw:
    """Not a token of any valid stream: "l" a litlen symbol, "d" a distance symbol with extra bits,
    "bits" plain bits. The builder does not expand it; the case states what the record decodes to."""

    def __init__(self, what, a, n=0, v=0):
        self.what, self.a, self.n, self.v = what, a, n, v


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 32
_FIXED = (canonical(FIXED_LL), canonical(FIXED_DL))
_RNG = random.Random(0xDEF1A7E)  # auto code choices (flat_lengths) when a case passes no rng


def plain_rle(seq):
    return list(seq)


def expand_rle(items):
    out = []
    for it in items:
        if isinstance(it, int):
            out.append(it)
        elif it[0] == 16:
            out += [out[-1]] * it[1]
        else:
            out += [0] * it[1]
    return out


def _dyn_header(w, b, toks, rng):
    used_l, used_d = {256}, set()
    for t in toks:
        if isinstance(t, int):
            used_l.add(t)
        elif isinstance(t, tuple):
            used_l.add(len_sym(t[0], len(t) > 2)[0])
            used_d.add(dist_sym(t[1])[0])
        elif t.what == "len":
            used_l.add(len_sym(t.a)[0])
    ll = b.ll
    if ll is None:
        if len(used_l) == 1:
            used_l.add(0)
        ll = flat_lengths(used_l, max(257, max(used_l) + 1), rng)
    dl = b.dl
    if dl is None:
        if len(used_d) < 2:
            used_d |= {0, 1}
        dl = flat_lengths(used_d, max(used_d) + 1, rng)
    items = b.rle if b.rle is not None else plain_rle(ll + dl)
    cl = b.cl
    if cl is None:
        syms = {it if isinstance(it, int) else it[0] for it in items}
        if len(syms) == 1:
            syms.add(0 if 0 not in syms else 8)
        cl = flat_lengths(syms, 19, rng)
    hclen = b.hclen if b.hclen is not None else max(4, max(i + 1 for i, s in enumerate(ORDER) if cl[s]))
    w.put(b.hlit if b.hlit is not None else len(ll) - 257, 5)
    w.put(b.hdist if b.hdist is not None else len(dl) - 1, 5)
    w.put(hclen - 4, 4)
    for s in ORDER[:hclen]:
        w.put(cl[s], 3)
    cc = canonical(cl)
    for it in items:
        if isinstance(it, int):
            w.code(cc[it])
        else:
            w.code(cc[it[0]])
            base, nb = {16: (3, 2), 17: (3, 3), 18: (11, 7)}[it[0]]
            w.put(it[1] - base, nb)
    return canonical(ll), canonical(dl)


def deflate(tokens, rng=None):
    """(raw DEFLATE bytes, the bytes the tokens expand to) of one member's token list."""
    rng = rng or _RNG
    blocks = []
    for t in tokens:
        if isinstance(t, Blk):
            blocks.append((t, []))
        else:
            blocks[-1][1].append(t)
    w, out = Bits(), bytearray()
    for bi, (b, toks) in enumerate(blocks):
        w.put(1 if (b.final if b.final is not None else bi == len(blocks) - 1) else 0, 1)
        w.put({"stored": 0, "fixed": 1, "dyn": 2, "bad": 3}[b.kind], 2)
        if b.kind == "stored":
            data = bytes(toks)
            w.align()
            ln = len(data) if b.ln is None else b.ln
            w.raw(struct.pack("<HH", ln, (ln ^ 0xFFFF) if b.nlen is None else b.nlen))
            w.raw(data)
            out += data
            continue
        lc, dc = _FIXED if b.kind == "fixed" else _dyn_header(w, b, toks, rng)
        for t in toks:
            if isinstance(t, int):
                w.code(lc[t])
                out.append(t)
            elif isinstance(t, tuple):
                ln, dist = t[0], t[1]
                s, eb, ev = len_sym(ln, len(t) > 2)
                w.code(lc[s])
                w.put(ev, eb)
                s, eb, ev = dist_sym(dist)
                w.code(dc[s])
                w.put(ev, eb)
                assert dist <= len(out)
                if dist >= ln:
                    out += out[len(out) - dist:len(out) - dist + ln]
                else:
                    out += (bytes(out[-dist:]) * (ln // dist + 1))[:ln]
            elif t.what == "l":
                w.code(lc[t.a])
            elif t.what == "d":
                w.code(dc[t.a])
                w.put(t.v, t.n)
            elif t.what == "len":  # a length symbol alone (the distance follows as Raw "d")
                s, eb, ev = len_sym(t.a)
                w.code(lc[s])
                w.put(ev, eb)
            else:
                w.put(t.a, t.n)
        if not (toks and isinstance(toks[-1], Raw) and toks[-1].what == "noeob"):
            w.code(lc[256])
    w.align()
    return bytes(w.out), bytes(out)


def trailer(data, isize=None, crc=None):
    return struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF if crc is None else crc,
                       len(data) & 0xFFFFFFFF if isize is None else isize)


def gz(members, rng=None, isize=None):
    """(payload, expected bytes) of a record of one or more members (token lists). isize: overrides the
    last member's ISIZE (the expected result is then the case's business)."""
    pay, out = bytearray(), bytearray()
    for k, toks in enumerate(members):
        body, data = deflate(toks, rng)
        pay += corpus.gzip_header() + body + trailer(data, isize if k == len(members) - 1 else None)
        out += data
    return bytes(pay), bytes(out)


# ---- tracer ---------------------------------------------------------------------------------------
class Corrupt(Exception):
    pass


class _Huff:
    def __init__(self, lengths, name):
        self.name = name
        self.cnt = [0] * 16
        for ln in lengths:
            self.cnt[ln] += 1
        self.cnt[0] = 0
        self.empty = not any(self.cnt)
        self.sym = [s for ln in range(1, 16) for s, v in enumerate(lengths) if v == ln]
        if self.empty:
            return
        mx = max(ln for ln in range(16) if self.cnt[ln])
        code = 0
        for ln in range(1, mx + 1):
            code = (code << 1) + self.cnt[ln]
        # complete, or Go's exception (huffmanDecoder.init): a single code of one bit
        if code != 1 << mx and not (code == 1 and mx == 1):
            raise Corrupt(f"{name} code {'over-subscribed' if code > 1 << mx else 'incomplete'}")
        self.single = code == 1 and mx == 1


class _In:
    def __init__(self, data):
        self.d, self.p, self.end = data, 0, 8 * len(data)

    def bits(self, n):
        v = 0
        if n:
            q = self.p >> 3
            v = (int.from_bytes(self.d[q:q + 4], "little") >> (self.p & 7)) & ((1 << n) - 1)
            self.p += n
            if self.p > self.end:
                raise Corrupt("unexpected EOF")
        return v

    def sym(self, h):
        code = first = index = 0
        for ln in range(1, 16):
            code |= self.bits(1)
            c = h.cnt[ln]
            if code - first < c:
                return h.sym[index + code - first], ln
            index += c
            first = (first + c) << 1
            code <<= 1
        raise Corrupt(f"no {h.name} code matches")


def trace(payload):
    """(bytes or CORRUPT, labels) of one record's gzip payload by Go's rules."""
    lab = set()
    try:
        return _gunzip(payload, lab), lab
    except Corrupt as e:
        lab.add(f"refused: {e}")
        return CORRUPT, lab


def _gunzip(pay, lab):
    if not pay:
        raise Corrupt("empty payload")  # (gzip.NewReader's bare io.EOF; the oracle's EOF class)
    s, out, members = _In(pay), bytearray(), 0
    while True:
        q = s.p >> 3
        if len(pay) - q < 10 or pay[q:q + 3] != b"\x1f\x8b\x08":
            raise Corrupt("member header")
        if pay[q + 3] & 0x1E:
            raise NotImplementedError("optional header fields are tests/corpus.py's business")
        s.p += 80
        dm = len(out)
        _inflate(s, out, dm, lab, members)
        s.p = (s.p + 7) & ~7
        q = s.p >> 3
        if len(pay) - q < 8:
            raise Corrupt("trailer")
        crc, isize = struct.unpack_from("<II", pay, q)
        if crc != zlib.crc32(bytes(out[dm:])) & 0xFFFFFFFF or isize != (len(out) - dm) & 0xFFFFFFFF:
            raise Corrupt("checksum")
        s.p += 64
        members += 1
        if s.p == s.end:
            lab.add(f"members={members}")
            return bytes(out)


def _token(s, lab, start):
    bits = s.p - start
    lab.add(f"tok{bits}")
    a, b = start >> 3, (s.p - 1) >> 3  # first and last payload byte the token has bits in
    if a < b:
        for m, name in ((1024, "x1024"), (128, "x128")):
            if (a // m) != (b // m):
                lab.add(name)


def _inflate(s, out, dm, lab, member):
    blocks, kinds, run1 = 0, set(), 0
    while True:
        h0 = s.p
        final, kind = s.bits(1), s.bits(2)
        blocks += 1
        kinds.add(kind)
        if kind == 3:
            raise Corrupt("block type 3")
        if kind == 0:
            s.p = (s.p + 7) & ~7
            ln, nl = s.bits(16), s.bits(16)
            if nl != ln ^ 0xFFFF:
                raise Corrupt("NLEN")
            q = s.p >> 3
            if q + ln > len(s.d):
                raise Corrupt("stored past the payload")
            out += s.d[q:q + ln]
            s.p += 8 * ln
            lab |= {f"st{ln}", f"stat{h0 & 7}"}
            if ln == 0:
                lab.add("st0final" if final else "st0open")
        else:
            if kind == 1:
                hl, hd = _Huff(FIXED_LL, "litlen"), _Huff(FIXED_DL, "distance")
            else:
                hl, hd = _dynamic(s, lab)
            while True:
                t0 = s.p
                v, n = s.sym(hl)
                lab.add(f"ll={n}")
                if getattr(hl, "single", False):
                    lab.add("one_ll_code")
                if n == 1 and v < 256:
                    run1 += 1
                else:
                    if run1 >= 300:
                        lab.add("lit1run>=300")
                    if run1 >= 300:
                        lab.add(f"brk{t0 & 63}")
                    run1 = 0
                if v < 256:
                    out.append(v)
                    _token(s, lab, t0)
                    continue
                if v == 256:
                    break
                if v > 285:
                    raise Corrupt("litlen symbol 286 / 287")
                ln = LBASE[v - 257] + s.bits(LEXTRA[v - 257])
                if v == 284 and ln == 258:
                    lab.add("m258via284")
                if kind == 1:
                    ds, dn = int(format(s.bits(5), "05b")[::-1], 2), 5
                else:
                    if hd.empty:
                        raise Corrupt("match under an empty distance code")
                    ds, dn = s.sym(hd)
                    if getattr(hd, "single", False):
                        lab.add("one_dist_code")
                lab.add(f"dl={dn}")
                if ds >= 30:
                    raise Corrupt("distance symbol 30 / 31")
                ev = s.bits(DEXTRA[ds])
                dist = DBASE[ds] + ev
                if ev == 0:
                    lab.add(f"ds{ds}lo")
                if ev == (1 << DEXTRA[ds]) - 1:
                    lab.add(f"ds{ds}hi")
                d = len(out)
                if dist > d - dm:
                    raise Corrupt("distance beyond the member's output")
                _token(s, lab, t0)
                lab.add(f"m{ln}@{dist}")
                if dist == d - dm:
                    lab.add("full@member" if member else "full@break" if blocks > 1 else "full@first")
                if dist == 32768 and d > 65536:
                    lab.add("d32768@>65536")
                for m in (1024, 32768):
                    if (d - dist) // m != (d - dist + ln - 1) // m:
                        lab.add(f"srcx{m}")
                    if d // m != (d + ln - 1) // m:
                        lab.add(f"dstx{m}")
                if dist >= ln:
                    out += out[d - dist:d - dist + ln]
                else:
                    out += (bytes(out[-dist:]) * (ln // dist + 1))[:ln]
        if final:
            lab.add(f"blocks{blocks}")
            if len(kinds) == 3:
                lab.add("types3")
            return


def _dynamic(s, lab):
    nlit, ndist, nclen = s.bits(5) + 257, s.bits(5) + 1, s.bits(4) + 4
    if nlit > 286:
        raise Corrupt("HLIT")
    if ndist > 30:
        raise Corrupt("HDIST")
    lab |= {f"hlit{nlit}", f"hdist{ndist}", f"hclen{nclen}"}
    cl = [0] * 19
    for k in range(nclen):
        cl[ORDER[k]] = s.bits(3)
    hc = _Huff(cl, "code-length")
    lens, total, plain, same = [], nlit + ndist, 0, 0
    prev_sym = None
    while len(lens) < total:
        x, n = s.sym(hc)
        lab.add(f"cl={n}")
        if x < 16:
            lens.append(x)
            plain += 1
            same = same + 1 if n == 1 and prev_sym == x else (1 if n == 1 else 0)
            if plain > 64:
                lab.add("plain>64")
            if same >= 130:
                lab.add("cl1run>=130")
            prev_sym = x
            continue
        plain = same = 0
        if x == 16:
            if not lens:
                raise Corrupt("repeat with nothing before it")
            rep, val = 3 + s.bits(2), lens[-1]
            if prev_sym in (17, 18):
                lab.add(f"r16after{prev_sym}")
        elif x == 17:
            rep, val = 3 + s.bits(3), 0
        else:
            rep, val = 11 + s.bits(7), 0
        if len(lens) + rep > total:
            raise Corrupt("run past HLIT + HDIST")
        lab.add(f"r{x}x{rep}")
        if len(lens) < nlit < len(lens) + rep:
            lab.add(f"cross{x}")
        if len(lens) + rep == total:
            lab.add(f"end{x}")
        lens += [val] * rep
        prev_sym = x
    hl, hd = _Huff(lens[:nlit], "litlen"), _Huff(lens[nlit:], "distance")
    if hd.empty:
        lab.add("empty_dist")
    return hl, hd


# ---- cases ----------------------------------------------------------------------------------------
class Case:
    """One record: its payload, what it decodes to (bytes or CORRUPT), and the header's u."""

    def __init__(self, name, payload, expect, u=None):
        self.name, self.payload, self.expect = name, payload, expect
        self.u = u if u is not None else (len(expect) if expect is not CORRUPT else 0)

    @property
    def valid(self):
        return self.expect is not CORRUPT

    @property
    def item(self):
        return (self.u, self.payload)


class Family:
    def __init__(self, name, cases, labels, refused=False, per_case=None):
        self.name, self.cases, self.labels, self.refused = name, cases, set(labels), refused
        self.per_case = per_case or {}  # case name -> labels that very case must produce


def ok(name, members, rng=None):
    pay, data = gz(members if isinstance(members[0], list) else [members], rng)
    return Case(name, pay, data)


def bad(name, members, rng=None, u=7, isize=None):
    pay, _ = gz(members if isinstance(members[0], list) else [members], rng, isize=isize)
    return Case(name, pay, CORRUPT, u)


def fill(rng, alphabet, n):
    return [rng.choice(alphabet) for _ in range(n)]


def code_length_family(seed=1):
    """Litlen and distance codes of every length 1..15, the fast tables' boundary pairs and a 7-bit
    code-length code, once per size class (<= 1024, 1025..2048, > 2048 decoded bytes)."""
    rng = random.Random(seed)
    cases = []

    def pad(toks, n, target, dsyms, ln=258):
        while n + ln <= target:
            toks.append((ln, DBASE[rng.choice(dsyms)]))
            n += ln
        return toks

    for cls, target in enumerate((800, 1600, 5000)):
        # 16 litlen symbols with lengths 1..14, 15, 15: 12 literals, EOB, three length symbols
        lits = rng.sample(range(256), 12)
        ll = shaped(lits + [256, 257, 258, 259], stair(14), 286, rng)
        dsyms = rng.sample(range(0, 18), 16)  # distances <= 512
        dl = shaped(dsyms, stair(14), max(dsyms) + 1, rng)
        toks, n = [Blk("dyn", ll=ll, dl=dl)] + lits * 44, 528  # every literal length, and room to reach back
        for k, ds in enumerate(dsyms):  # every distance code length
            ln = (3, 4, 5)[k % 3]
            toks.append((ln, DBASE[ds] + rng.randrange(1 << DEXTRA[ds])))
            n += ln
        cases.append(ok(f"len1to15_cls{cls}", pad(toks, n, target, dsyms, 5), rng))
        # boundary pairs around the fast tables: litlen 9 / 10, distance 7 / 8 and 9 / 10
        for nm, lshape, dshape in (("ll9_10_d7_8", stair(9), stair(7)), ("d9_10", stair(4), stair(9))):
            lits = rng.sample(range(256), len(lshape) - 3)
            ll = shaped(lits + [256, 257, 285], lshape, 286, rng)
            dsyms = rng.sample(range(0, 18), len(dshape))
            dl = shaped(dsyms, dshape, max(dsyms) + 1, rng)
            toks, n = [Blk("dyn", ll=ll, dl=dl)], 0
            while n < 520:
                toks += lits
                n += len(lits)
            for ds in dsyms * 2:
                toks.append((3, DBASE[ds] + rng.randrange(1 << DEXTRA[ds])))
                n += 3
            cases.append(ok(f"{nm}_cls{cls}", pad(toks, n, target, dsyms), rng))
        # a code-length code with 7-bit codes: the header carries the lengths 0..7, coded 1..6, 7, 7
        cl = shaped(list(range(8)), stair(6), 19, rng, pin={0: 1})
        lits = rng.sample(range(256), 6)
        ll = [0] * 286
        for s, ln in zip(lits + [256, 285], stair(6)):
            ll[s] = ln
        toks = [Blk("dyn", ll=ll, dl=[1, 1], cl=cl)] + fill(rng, lits, 300)
        cases.append(ok(f"clen7_cls{cls}", pad(toks, 300, target, [0, 1]), rng))
    labels = {f"ll={n}" for n in range(1, 16)} | {f"dl={n}" for n in range(1, 16)} | {"cl=7"}
    sizes = {c.name: len(c.expect) for c in cases}
    assert all((v <= 1024, 1024 < v <= 2048, v > 2048)[int(k[-1])] for k, v in sizes.items()), sizes
    per = {f"len1to15_cls{c}": labels - {"cl=7"} for c in range(3)}
    per.update({f"ll9_10_d7_8_cls{c}": {"ll=9", "ll=10", "dl=7", "dl=8"} for c in range(3)})
    per.update({f"d9_10_cls{c}": {"dl=9", "dl=10"} for c in range(3)})
    per.update({f"clen7_cls{c}": {"cl=7"} for c in range(3)})
    return Family("code_lengths", cases, labels, per_case=per)


def header_family(seed=2):
    """Dynamic headers: HLIT / HDIST / HCLEN at their ends, every repeat symbol at its lowest and
    highest count, runs across the litlen / distance boundary and up to the last length."""
    rng = random.Random(seed)
    cases, per = [], {}

    def add(name, toks, labels):
        cases.append(ok(name, toks, rng))
        per[name] = set(labels)

    text = fill(rng, list(b"header codings "), 200)
    # HLIT 257, HDIST 1, HCLEN 5: symbols 1..256 with eight bits each and an empty distance code; the
    # code-length code has two one-bit codes (0 and 8), so 8 comes 256 times in a row as a one-bit code.
    # (HCLEN 4 carries lengths for 16, 17, 18 and 0 only, so every litlen length is zero and the block
    # cannot end: refused_family has it.)
    cl = [0] * 19
    cl[8] = cl[0] = 1
    add("hlit257_hdist1_hclen5", [Blk("dyn", ll=[0] + [8] * 256, dl=[0], cl=cl)] + [1 + (b % 255) for b in text],
        {"hlit257", "hdist1", "hclen5", "plain>64", "cl1run>=130", "empty_dist"})
    # HLIT 286, HDIST 30, HCLEN 19 (the code-length code's last symbol in the order, 15, has a code)
    ll = shaped(list(range(286)), [8] * 226 + [9] * 60, 286, rng)
    dl = shaped(list(range(30)), [4] * 2 + [5] * 28, 30, rng)
    cl = flat_lengths(set(ll + dl) | {15, 1}, 19, rng)
    add("hlit286_hdist30_hclen19", [Blk("dyn", ll=ll, dl=dl, cl=cl)] + text + [(10, 7), (258, 200)],
        {"hlit286", "hdist30", "hclen19", "plain>64"})
    # every repeat count at its ends; 16 straight after 17 and after 18 repeats their zero. Symbols
    # 0..32 zero, 33..43 eight bits, 44..181 zero, 182 one bit, 183..196 seven bits, 197..285 eight bits
    items = [(17, 3), (16, 3), (18, 11), (16, 6), (17, 10), 8, (16, 3), 8, (16, 6), (18, 138)] + [1] + [7] * 14 + [8] * 89
    seq = expand_rle(items)
    assert len(seq) == 286 and kraft(seq) == 32768
    lits = [s for s in range(256) if seq[s]]
    add("repeat_counts", [Blk("dyn", ll=seq, dl=[1, 1], rle=items + [1, 1])] + fill(rng, lits, 300) + [(258, 2)],
        {"r17x3", "r16x3", "r18x11", "r16x6", "r17x10", "r18x138", "r16after17", "r16after18", "plain>64"})
    # a 16-run across the boundary and one that ends at HLIT + HDIST: litlen 250..257 and distance 0..7
    # with three bits each
    items = [(18, 138), (18, 112), 3, (16, 6), (16, 6), (16, 3)]
    seq = expand_rle(items)
    assert len(seq) == 258 + 8 and seq[250:] == [3] * 16
    add("cross16_end16", [Blk("dyn", ll=seq[:258], dl=seq[258:], rle=items)] + fill(rng, list(range(250, 256)), 100) +
        [(3, 9), (3, 16), (3, 1)], {"cross16", "end16", "r18x138"})
    # an 18-run across the boundary (litlen 258..269 and distance 0..11 zero) and a 17-run up to the end
    items = [(18, 138), (18, 104)] + [4] * 16 + [(18, 24)] + [1, 1] + [(17, 3)]
    seq = expand_rle(items)
    assert len(seq) == 270 + 17 and seq[242:258] == [4] * 16
    add("cross18_end17", [Blk("dyn", ll=seq[:270], dl=seq[270:], rle=items)] + fill(rng, list(range(242, 256)), 110) +
        [(3, DBASE[12]), (3, DBASE[13] + 5)], {"cross18", "end17"})
    items = [(18, 138), (18, 104)] + [4] * 16 + [1, 1] + [(18, 11)]
    seq = expand_rle(items)
    add("end18", [Blk("dyn", ll=seq[:258], dl=seq[258:], rle=items)] + fill(rng, list(range(242, 256)), 60) + [(3, 2)],
        {"end18"})
    return Family("header_codings", cases, set().union(*per.values()), per_case=per)


def one_bit_literal_family(seed=3):
    """A literal with a one-bit code in runs of 300 and more (the run lookup's 64 bit offsets all hold
    literals), broken by deeper symbols; records are added until a run has ended at every bit phase."""
    rng = random.Random(seed)
    cases, labels = [], {"lit1run>=300"} | {f"brk{p}" for p in range(64)}
    seen = set()
    while not labels <= seen:
        a = rng.randrange(256)
        others = rng.sample([b for b in range(256) if b != a], 5)
        ll = shaped([a] + others + [256, 285], stair(6), 286, rng, pin={a: 1})
        toks = [Blk("dyn", ll=ll, dl=[1, 1])]
        for _ in range(16):
            toks += [a] * rng.randint(300, 363) + [rng.choice(others)]
        toks += [(258, 1)] if len(cases) % 2 else []
        cases.append(ok(f"one_bit_{len(cases)}", toks, rng))
        seen |= _labels_of(cases[-1])
        assert len(cases) < 40
    return Family("one_bit_literal", cases, labels)


LARGE_DISTS = list(range(1, 265)) + [511, 512, 513, 1023, 1024, 1025, 4095, 4096, 16384, 32767, 32768]
SMALL_LENS = (3, 4, 15, 16, 17, 63, 64, 65, 66, 127, 128, 129, 257, 258)


def _seed_bytes(rng, n):
    return [rng.randrange(256) for _ in range(n)]


def match_family(seed=4):
    rng = random.Random(seed)
    cases, labels = [], set()
    # large class: one record per distance, every length 3..258 (258 both ways); a stored head gives the
    # history cheaply, fixed blocks carry the matches (long records; dynamic tables add nothing here)
    for dist in LARGE_DISTS:
        head = _seed_bytes(rng, max(dist, 2100))
        lens = list(range(3, 259))
        rng.shuffle(lens)
        toks = [Blk("stored")] + head + [Blk("fixed")]
        for ln in lens:
            toks += [(ln, dist), rng.randrange(256)]
        toks.append((258, dist, "alt"))
        cases.append(ok(f"large_d{dist}", toks, rng))
        labels |= {f"m{ln}@{dist}" for ln in range(3, 259)}
    labels.add("m258via284")
    # tiny and small classes: distances 1..64 with the edge lengths, cut to fit the class
    for cls, cap in ((0, 1024), (1, 2048)):
        for dist in range(1, 65):
            toks, n = [Blk("dyn")] + _seed_bytes(rng, dist), dist
            if cls == 1:
                toks += _seed_bytes(rng, 200)
                n += 200
            lens = list(SMALL_LENS)
            rng.shuffle(lens)
            k = 0
            while True:  # the lengths round-robin over the distances' records: every pair within a few
                ln = lens[k % len(lens)]
                if n + ln + 1 > cap or k >= len(lens):
                    break
                toks += [(ln, dist), rng.randrange(256)]
                n += ln + 1
                k += 1
            while cls == 1 and n <= 1024:
                toks.append((258, dist))
                n += 258
            cases.append(ok(f"cls{cls}_d{dist}", toks, rng))
    # the pairs a single record could not hold (1024 / 2048 bytes) go to a second record per distance
    for cls, cap in ((0, 1024), (1, 2048)):
        for dist in range(1, 65):
            got = set()
            for c in cases:
                if c.name == f"cls{cls}_d{dist}":
                    got = {ln for ln in SMALL_LENS if _has_pair(c, ln, dist)}
            rest = [ln for ln in SMALL_LENS if ln not in got]
            part = 0
            while rest:
                toks, n = [Blk("fixed")] + _seed_bytes(rng, dist), dist
                if cls == 1:
                    toks += _seed_bytes(rng, 1025 - min(1025, dist))
                    n = max(n, 1025)
                while rest and n + rest[0] <= cap:
                    toks.append((rest[0], dist))
                    n += rest.pop(0)
                cases.append(ok(f"cls{cls}_d{dist}_more{part}", toks, rng))
                part += 1
    # every distance symbol at its lowest and highest extra bits (32 KiB of stored history first)
    toks = [Blk("stored")] + _seed_bytes(rng, 32768) + [Blk("dyn")]
    for s in range(30):
        toks += [(3 + s, DBASE[s]), (4 + s, DBASE[s] + (1 << DEXTRA[s]) - 1)]
        labels |= {f"ds{s}lo", f"ds{s}hi"}
    cases.append(ok("all_distance_symbols", toks, rng))
    # distance = everything the member has produced: first block, after a block break, second member
    a, b = _seed_bytes(rng, 300), _seed_bytes(rng, 77)
    cases.append(ok("full_first", [Blk("fixed")] + a + [(258, 300)], rng))
    cases.append(ok("full_break", [Blk("fixed")] + a + [Blk("dyn")] + b + [(100, 377)], rng))
    cases.append(ok("full_member", [[Blk("fixed")] + a, [Blk("fixed")] + b + [(77, 77), (3, 154)]], rng))
    cases.append(ok("full_first_large", [Blk("stored")] + _seed_bytes(rng, 3000) + [Blk("fixed"), (258, 3000)], rng))
    cases.append(ok("full_member_large", [[Blk("stored")] + _seed_bytes(rng, 2500),
                                          [Blk("stored")] + _seed_bytes(rng, 1030) + [Blk("fixed"), (200, 1030)]], rng))
    labels |= {"full@first", "full@break", "full@member"}
    # distance 32768 past position 65536, and matches straddling multiples of 32768 and 1024
    toks = [Blk("stored")] + _seed_bytes(rng, 32768) + [Blk("fixed")]
    n = 32768
    while n < 3 * 32768 + 5000:
        at = n % 32768
        if at > 32768 - 300 or at < 300:
            ln, dist = rng.choice([3, 64, 65, 258]), rng.choice([32768, 32767, 32768 - 63, 32768 - 64, 1, 300])
        else:
            ln, dist = rng.randint(3, 258), rng.choice([32768, 32768, 32767, rng.randint(1, 32768)])
        toks.append((ln, dist))
        n += ln
        if rng.random() < 0.2:
            toks.append(rng.randrange(256))
            n += 1
    cases.append(ok("window_wrap", toks, rng))
    labels |= {"d32768@>65536", "srcx32768", "dstx32768", "srcx1024", "dstx1024"}
    return Family("matches", cases, labels)


def _has_pair(case, ln, dist):
    return f"m{ln}@{dist}" in _labels_of(case)


_TRACED = {}


def traced(case):
    """trace(case.payload), computed once per case."""
    k = id(case)
    if k not in _TRACED or _TRACED[k][0] is not case:
        _TRACED[k] = (case,) + trace(case.payload)
    return _TRACED[k][1:]


def _labels_of(case):
    return traced(case)[1]


def stored_family(seed=5):
    rng = random.Random(seed)
    cases, labels = [], set()
    cases.append(ok("len0_final", [Blk("fixed")] + list(b"abc") + [Blk("stored")], rng))
    cases.append(ok("len0_open", [Blk("stored"), Blk("fixed")] + list(b"abc") + [Blk("stored"), Blk("stored")], rng))
    cases.append(ok("len0_only", [Blk("stored")], rng))
    labels |= {"st0final", "st0open"}
    for ln in (1, 1023, 1024, 1025, 65535):
        cases.append(ok(f"len{ln}", [Blk("stored")] + _seed_bytes(rng, ln), rng))
        cases.append(ok(f"len{ln}_after", [Blk("fixed")] + list(b"xy") + [Blk("stored")] + _seed_bytes(rng, ln) +
                        [Blk("fixed"), (20, min(ln, 32768)), (3, 1)], rng))
        labels.add(f"st{ln}")
    # a stored block after a fixed block that ends at each bit offset: fixed literals < 144 take 8 bits,
    # >= 144 take 9, EOB 7; the stored header starts where the EOB ends
    seen = set()
    for nine in range(16):
        toks = [Blk("fixed")] + [200] * nine + [65] * 3 + [Blk("stored")] + _seed_bytes(rng, 40) + [Blk("fixed"), (30, 35)]
        c = ok(f"misaligned_{nine}", toks, rng)
        at = {x for x in _labels_of(c) if x.startswith("stat")}
        if not at <= seen:
            cases.append(c)
            seen |= at
    labels |= {f"stat{k}" for k in range(8)}
    # stored / Huffman / stored, matches reaching back into stored bytes
    for k, total in enumerate((900, 1900, 9000)):
        toks, n = [], 0
        while n < total:
            m = rng.randint(20, 120)
            toks += [Blk("stored")] + _seed_bytes(rng, m)
            n += m
            toks.append(Blk(rng.choice(["fixed", "dyn"])))
            for _ in range(3):
                ln = rng.randint(3, 40)
                toks += [(ln, rng.randint(1, n)), rng.randrange(256)]
                n += ln + 1
        cases.append(ok(f"alternating_{k}", toks, rng))
    # tiny class: stored payloads several times the input ring, with Huffman blocks in between
    toks = [Blk("stored")] + _seed_bytes(rng, 600) + [Blk("fixed"), (10, 600), (3, 1)] + [Blk("stored")] + \
        _seed_bytes(rng, 300) + [Blk("dyn"), (50, 913), 7, 8, (9, 2)]
    cases.append(ok("tiny_ring", toks, rng))
    return Family("stored", cases, labels)


def many_blocks_family(seed=6):
    rng = random.Random(seed)
    eob_only = dict(ll=[0] * 256 + [1], dl=[0], rle=[(18, 138), (18, 118), 1, 0])  # litlen: the single one-bit EOB
    cases = []
    for tail in (0, 3):
        data = _seed_bytes(rng, tail)
        cases.append(ok(f"empty_fixed_{tail}", [Blk("fixed")] * 3000 + [Blk("stored")] + data, rng))
        cases.append(ok(f"empty_dyn_{tail}", [Blk("dyn", **eob_only)] * 3000 + [Blk("fixed")] + data, rng))
    toks, n = [], 0
    for k in range(200):
        toks.append(Blk(("stored", "fixed", "dyn")[k % 3]))
        if k % 3 == 0:
            toks += _seed_bytes(rng, k % 7)
            n += k % 7
        elif k % 5:
            toks += _seed_bytes(rng, 2) + ([(3 + k % 9, rng.randint(1, n + 2))] if n else [])
            n += 2 + (3 + k % 9 if n else 0)
    cases.append(ok("rotating_200", toks, rng))
    cases.append(ok("empty_final", [Blk("fixed")] + list(b"data then an empty final block") + [Blk("fixed")], rng))
    labels = {"blocks3001", "blocks200", "types3", "one_ll_code", "empty_dist", "blocks2"}
    return Family("many_blocks", cases, labels)


def wide_token_family(seed=7):
    """Tokens of 15 + 5 + 15 + 13 bits (a 15-bit length code with 5 extra bits, a 15-bit distance code
    with 13) filling 8 KiB and 64 KiB of payload, so they straddle the 1 KiB refill blocks of the input
    ring at every phase; the tiny class (distances < 1 KiB, 128-byte blocks) gets 15 + 5 + 15 + 7."""
    rng = random.Random(seed)
    cases = []
    for name, pay_bytes in (("8k", 8192), ("64k", 65536)):
        lits = rng.sample(range(256), 12)
        ll = shaped(lits + [256, 283, 284, 285], stair(14), 286, rng, pin={283: 15, 284: 15})
        dsyms = [0] + rng.sample(range(1, 28), 13) + [28, 29]
        dl = shaped(dsyms, stair(14), 30, rng, pin={28: 15, 29: 15})
        # 32 KiB of history from a few tokens, then the wide ones (lengths 195..257: symbols 283, 284)
        toks = [Blk("dyn", ll=ll, dl=dl)] + lits + [(258, 1)] * 127
        toks += [(195 + rng.randrange(63), DBASE[rng.choice([28, 29])] + rng.randrange(8192))
                 for _ in range(pay_bytes * 8 // 48)]
        cases.append(ok(f"wide_{name}", toks, rng))
    lits = rng.sample(range(256), 13)
    ll = shaped(lits + [256, 281, 282], stair(14), 286, rng, pin={281: 15, 282: 15})
    dl = shaped(rng.sample(range(0, 16), 14) + [16, 17], stair(14), 18, rng, pin={16: 15, 17: 15})
    toks = [Blk("stored")] + _seed_bytes(rng, 520) + [Blk("dyn", ll=ll, dl=dl)]
    toks += [(131 + rng.randrange(32), DBASE[rng.choice([16, 17])] + rng.randrange(128)) for _ in range(3)]
    cases.append(ok("wide_tiny", toks, rng))
    # tiny class with a long payload: 15-bit literals only (1000 of them: 1875 payload bytes), so tokens
    # straddle the 128-byte refill blocks of its input ring at many phases
    lits = rng.sample(range(256), 14)
    ll = shaped(lits + [256, 285], stair(14), 286, rng)
    long15 = [s for s in lits if ll[s] >= 14]
    toks = [Blk("dyn", ll=ll, dl=[1, 1])] + fill(rng, long15, 1000)
    cases.append(ok("wide_tiny_literals", toks, rng))
    per = {"wide_8k": {"x1024", "tok48"}, "wide_64k": {"x1024", "tok48"}, "wide_tiny": {"tok42"},
           "wide_tiny_literals": {"x128", "ll=15"}}
    return Family("wide_tokens", cases, {"x1024", "x128", "tok48"}, per_case=per)


def accepted_family(seed=8):
    rng = random.Random(seed)
    text = fill(rng, list(b"go accepts this "), 120)
    cases = [
        ok("single_distance_code_used", [Blk("dyn", dl=[1])] + text + [(30, 1), (258, 1)], rng),
        ok("single_distance_code_second", [Blk("dyn", dl=[0, 0, 0, 1])] + text + [(30, 4), (9, 4)], rng),
        ok("empty_distance_code_unused", [Blk("dyn", dl=[0])] + text, rng),
        ok("empty_distance_code_long", [Blk("dyn", dl=[0] * 30)] + text, rng),
        ok("single_litlen_code", [Blk("dyn", ll=[0] * 256 + [1], dl=[0]), Blk("fixed")] + text, rng),
    ]
    return Family("accepted", cases, {"one_dist_code", "empty_dist", "one_ll_code"})


def refused_family(seed=9):
    rng = random.Random(seed)
    text = fill(rng, list(b"refused by go "), 60)
    eight = [0] + [8] * 256
    inc = [0] + [8] * 255 + [0]  # 255 codes of 8 bits and none for EOB .. incomplete
    over = [8] * 257
    cases = [
        # the unused bit of a single-code table: the only distance code is 0; a 1 bit matches nothing
        bad("single_code_other_bit", [Blk("dyn", dl=[1])] + text + [Raw("len", 10), Raw("bits", 1, 1)], rng),
        bad("single_ll_code_other_bit", [Blk("dyn", ll=[0] * 256 + [1], dl=[0]), Raw("bits", 1, 1), Raw("noeob", 0)], rng),
        bad("match_under_empty_distance", [Blk("dyn", dl=[0])] + text + [Raw("len", 10), Raw("bits", 0, 8)], rng),
        bad("litlen_incomplete", [Blk("dyn", ll=inc + [0], dl=[1, 1])] + text[:0] + [Raw("bits", 0, 16), Raw("noeob", 0)], rng),
        bad("litlen_oversubscribed", [Blk("dyn", ll=over, dl=[1, 1])] + [Raw("bits", 0, 16), Raw("noeob", 0)], rng),
        bad("dist_incomplete", [Blk("dyn", ll=eight, dl=[1, 2])] + [1, 2, 3], rng),
        bad("dist_two_bit_single", [Blk("dyn", ll=eight, dl=[2])] + [1, 2, 3], rng),
        bad("dist_oversubscribed", [Blk("dyn", ll=eight, dl=[1, 1, 1])] + [1, 2, 3], rng),
        bad("clen_incomplete", [Blk("dyn", ll=eight, dl=[1, 1], cl=_cl({0: 2, 8: 2, 1: 2}))] + [1, 2, 3], rng),
        bad("clen_oversubscribed", [Blk("dyn", ll=eight, dl=[1, 1], cl=_cl({0: 1, 8: 1, 1: 1}))] + [1, 2, 3], rng),
        bad("litlen_two_two_bit_codes", [Blk("dyn", ll=[2] + [0] * 255 + [2], dl=[0])] + [0, 0], rng),
        bad("hclen4_all_zero", [Blk("dyn", ll=[0] * 257, dl=[0], cl=_cl({0: 1, 18: 1}), hclen=4,
                                    rle=[(18, 138), (18, 120)]), Raw("bits", 0, 16), Raw("noeob", 0)], rng),
        bad("hlit287", [Blk("dyn", ll=eight + [0] * 30, dl=[1, 1], hlit=30)] + [1, 2, 3], rng),
        bad("hlit288", [Blk("dyn", ll=eight + [0] * 31, dl=[1, 1], hlit=31)] + [1, 2, 3], rng),
        bad("hdist31", [Blk("dyn", ll=eight, dl=[1, 1] + [0] * 29, hdist=30)] + [1, 2, 3], rng),
        bad("hdist32", [Blk("dyn", ll=eight, dl=[1, 1] + [0] * 30, hdist=31)] + [1, 2, 3], rng),
        # read as "repeat zero" the lengths would be three zeros and 256 eights, a complete code: only
        # the rule that a repeat needs a length before it refuses the record
        bad("first_symbol_16", [Blk("dyn", ll=[0] * 3 + [8] * 256, dl=[1, 1], cl=_cl({16: 2, 0: 2, 8: 2, 1: 2}),
                                    rle=[(16, 3)] + [8] * 256 + [1, 1])] + [3, 4, 5], rng),
        bad("run_one_past_total", [Blk("dyn", ll=eight, dl=[1, 1], cl=_cl({17: 2, 0: 2, 8: 2, 1: 2}),
                                       rle=[0] + [8] * 256 + [1, 1, (17, 3)], hdist=3)] + [1, 2, 3], rng),
        bad("fixed_symbol_286", [Blk("fixed")] + text + [Raw("l", 286)], rng),
        bad("fixed_symbol_287", [Blk("fixed")] + text + [Raw("l", 287)], rng),
        bad("fixed_distance_30", [Blk("fixed")] + text + [Raw("len", 5), Raw("d", 30)], rng),
        bad("fixed_distance_31", [Blk("fixed")] + text + [Raw("len", 5), Raw("d", 31)], rng),
        bad("distance_one_past_output", [Blk("fixed")] + text + [Raw("len", 5), Raw("d", *_d(61))], rng),
        bad("distance_one_past_member", [[Blk("fixed")] + text, [Blk("fixed")] + text[:20] + [Raw("len", 5), Raw("d", *_d(21))]], rng),
    ]
    cases[-1].u = 80
    # (the run that ends one past total: HDIST says 4 distance lengths, the items give 2 + 3)
    body, data = deflate([Blk("stored", nlen=(40 ^ 0xFFFF) ^ 0x10)] + _seed_bytes(rng, 40))
    cases.append(Case("nlen_off_by_a_bit", corpus.gzip_header() + body + trailer(data), CORRUPT, 40))
    body, data = deflate([Blk("stored", ln=41)] + _seed_bytes(rng, 40))
    # LEN one past the payload: the 40 bytes and the trailer are 48 < 41 + 8; without a trailer it is 40 < 41
    cases.append(Case("len_one_past_payload", corpus.gzip_header() + body[:5] + body[5:5 + 40], CORRUPT, 40))
    why = {"single_code_other_bit": "no distance code matches", "single_ll_code_other_bit": "no litlen code matches",
           "match_under_empty_distance": "match under an empty distance code",
           "litlen_incomplete": "litlen code incomplete", "litlen_oversubscribed": "litlen code over-subscribed",
           "dist_incomplete": "distance code incomplete", "dist_two_bit_single": "distance code incomplete",
           "dist_oversubscribed": "distance code over-subscribed", "clen_incomplete": "code-length code incomplete",
           "clen_oversubscribed": "code-length code over-subscribed", "litlen_two_two_bit_codes": "litlen code incomplete",
           "hclen4_all_zero": "no litlen code matches", "hlit287": "HLIT", "hlit288": "HLIT", "hdist31": "HDIST",
           "hdist32": "HDIST", "first_symbol_16": "repeat with nothing before it",
           "run_one_past_total": "run past HLIT + HDIST", "fixed_symbol_286": "litlen symbol 286 / 287",
           "fixed_symbol_287": "litlen symbol 286 / 287", "fixed_distance_30": "distance symbol 30 / 31",
           "fixed_distance_31": "distance symbol 30 / 31", "distance_one_past_output": "distance beyond the member's output",
           "distance_one_past_member": "distance beyond the member's output", "nlen_off_by_a_bit": "NLEN",
           "len_one_past_payload": "stored past the payload"}
    assert set(why) == {c.name for c in cases}
    per = {k: {f"refused: {v}"} for k, v in why.items()}  # refused by the rule the case is about, not by accident
    return Family("refused", cases, set(), refused=True, per_case=per)


def _cl(d):
    out = [0] * 19
    for s, ln in d.items():
        out[s] = ln
    return out


def _d(dist):
    s, eb, ev = dist_sym(dist)
    return s, eb, ev


def cut_body_family(seed=10):
    rng = random.Random(seed)
    words = [bytes(rng.choice(b"abcdefghij") for _ in range(rng.randint(2, 6))) for _ in range(12)]
    text = b" ".join(rng.choice(words) for _ in range(95))
    co = zlib.compressobj(9, zlib.DEFLATED, -15)
    body = co.compress(text) + co.flush()
    assert body[0] & 6 == 4 and 130 <= len(body) <= 200, len(body)  # one dynamic block
    cases = []
    for cut in range(len(body)):
        pay = corpus.gzip_header() + body[:cut] + trailer(text)
        cases.append(Case(f"cut_{cut}", pay, None, len(text)))  # expectation: the tracer's (set by the CPU test's check)
    for c in cases:  # (a cut stream may still end in an end-of-block by chance: the tracer says)
        c.expect = traced(c)[0]
    cases.append(Case("uncut", corpus.gzip_header() + body + trailer(text), text))
    return Family("cut_bodies", cases, set(), refused=True)


def cap_family(seed=11):
    """Records of two members: the first decode pass caps the output at the last member's ISIZE, and
    each token kind meets that cap exactly or overshoots it by one; then single members whose ISIZE
    lies (corrupt by the size check; the point is the class change between the two rounds)."""
    rng = random.Random(seed)
    cases = []
    lits = list(b"capcrossing")
    for cap in (40, 1100, 2100):  # the last member's size = the cap: each class
        second = [Blk("stored")] + _seed_bytes(rng, cap)
        for over in (0, 1):
            n = cap + over  # the first member alone reaches n: the cap exactly, or one past it
            # literal inside a run (G = 64: a run of fast-table literals), lone literal after a match
            first = {
                "run": [Blk("fixed")] + fill(rng, lits, n) + [Blk("fixed")] + fill(rng, lits, 9),
                "lone": [Blk("fixed")] + fill(rng, lits, 8) + [(n - 9, 3), 66] + [Blk("fixed"), 1, 2],
                "match": [Blk("fixed")] + fill(rng, lits, 8) + [(n - 8, 5)] + [Blk("fixed"), 1, 2],
                "stored": [Blk("fixed")] + fill(rng, lits, 8) + [Blk("stored")] + _seed_bytes(rng, n - 8) + [Blk("fixed"), 3],
            }
            for kind, toks in first.items():
                toks = _split_long(toks)
                cases.append(ok(f"cap{cap}_{kind}_{'over' if over else 'exact'}", [toks, second], rng))
    # ISIZE lies
    for real, claim in ((1500, 10), (40000, 10), (10, 40000)):
        toks = [Blk("stored")] + _seed_bytes(rng, min(real, 50)) + [Blk("fixed")]
        n = min(real, 50)
        while n < real:
            ln = min(258, real - n)
            if ln < 3:
                toks += [0] * ln
            else:
                toks.append((ln, rng.randint(1, 40)))
            n += ln
        cases.append(bad(f"isize_{claim}_decodes_{real}", toks, rng, u=real, isize=claim))
    return Family("cap_crossings", cases, {"members=2"})


def _split_long(toks):
    out = []
    for t in toks:
        if isinstance(t, tuple) and t[0] > 258:
            ln, dist = t
            while ln > 258 + 2:
                out.append((258, dist))
                ln -= 258
            if ln > 258:
                out += [(ln - 3, dist), (3, dist)]
            else:
                out.append((ln, dist))
        else:
            out.append(t)
    return out


NEIGHBOUR_KINDS = ("stored", "fixed", "dyn15", "empty3000", "bad_magic", "corrupt_mid", "nil", "empty")


def neighbour_family(seed=12, groups=56):
    """Tiny-class records in aligned groups of four (one wave): every rotation of every choice of four
    kinds in a fixed cyclic order, so a record that fails at once or runs 100 times longer sits in each
    of the four positions beside ordinary ones."""
    rng = random.Random(seed)
    items = []
    lits = rng.sample(range(256), 13)
    ll15 = shaped(lits + [256, 257, 285], stair(14), 286, rng)

    def make(kind, k):
        data = _seed_bytes(rng, rng.randint(1, 300))
        if kind == "stored":
            return ok(f"n{k}_stored", [Blk("stored")] + data, rng)
        if kind == "fixed":
            return ok(f"n{k}_fixed", [Blk("fixed")] + data + [(rng.randint(3, 258), rng.randint(1, len(data)))], rng)
        if kind == "dyn15":
            return ok(f"n{k}_dyn15", [Blk("dyn", ll=ll15, dl=[1, 1])] + fill(rng, lits, 200) + [(258, 2), (3, 1)], rng)
        if kind == "empty3000":
            return ok(f"n{k}_empty3000", [Blk("fixed")] * 3000 + [Blk("stored")] + data[:5], rng)
        if kind == "bad_magic":
            c = ok(f"n{k}_bad_magic", [Blk("fixed")] + data, rng)
            return Case(c.name, b"\x1f\x8c" + c.payload[2:], CORRUPT, len(data))
        if kind == "corrupt_mid":
            pay, exp = gz([[Blk("fixed")] + data + [Raw("l", 286)] + data], rng)
            return Case(f"n{k}_corrupt_mid", pay, CORRUPT, len(data))
        if kind == "nil":
            return None
        return ok(f"n{k}_empty", [Blk("stored")], rng)

    k = 0
    for g in range(groups):
        four = [NEIGHBOUR_KINDS[(g + j * (1 + g // 8 % 3)) % 8] for j in range(4)]
        for rot in range(4):
            for j in range(4):
                items.append(make(four[(j + rot) % 4], k))
                k += 1
    return items


def cached(fn, _memo={}):
    if fn not in _memo:
        _memo[fn] = fn()
    return _memo[fn]


VALID_FAMILIES = (code_length_family, header_family, one_bit_literal_family, match_family, stored_family,
                  many_blocks_family, wide_token_family, accepted_family, cap_family)
REFUSED_FAMILIES = (refused_family, cut_body_family)


def families():
    return [cached(f) for f in VALID_FAMILIES + REFUSED_FAMILIES]


def good_records(n, seed):
    """Ordinary zlib-made records (as corpus.gzip_cases' `good`): the neighbours of a refused record."""
    text = corpus.text_records(n, seed, 1, 900)
    return [Case(f"good{i}", corpus.gzip_member(r), r) for i, r in enumerate(text)]


def family_files(fam):
    """[(name, gz image, cases in file order)]: valid families as a few files of at most ~6 MB decoded;
    refused ones with each bad record in the middle of good ones (as corpus.gzip_cases' corrupt())."""
    if fam.refused:
        good = good_records(4, 99)
        recs = []
        for c in fam.cases:
            recs += [good[0], good[1], c, good[2]]
        return [(fam.name, corpus.gz_file([c.item for c in recs]), recs)]
    files, cur, size = [], [], 0
    for c in fam.cases:
        if cur and size + len(c.expect) > 6 << 20:
            files.append(cur)
            cur, size = [], 0
        cur.append(c)
        size += len(c.expect)
    files.append(cur)
    return [(f"{fam.name}_{i}", corpus.gz_file([c.item for c in cs]), cs) for i, cs in enumerate(files)]


def shuffled_all(seed=77, large_matches=40):
    """Every family in one shuffled file (the tiny, small and large classes and the redo round in one
    decode); of the 275 large match records a seeded sample, to keep the file a few MB."""
    rng = random.Random(seed)
    cases = []
    for fam in families():
        cs = fam.cases
        if fam.name == "matches":
            big = [c for c in cs if c.name.startswith("large_d")]
            keep = set(id(c) for c in rng.sample(big, large_matches))
            cs = [c for c in cs if not c.name.startswith("large_d") or id(c) in keep]
        cases += cs
    cases += [c for c in neighbour_family(groups=8)]
    rng.shuffle(cases)
    items = [None if c is None else c.item for c in cases]
    return corpus.gz_file(items), cases


def redo_file(n=2500, every=50, seed=31):
    """(image, records, indices of the records of two members): zlib-made text records; every `every`-th
    is split into two gzip members, so the framing's size (the last member's ISIZE) is too small and the
    record goes through k_gz_resize and the redo round. Long enough for more than 1536 chunks of 256 bytes."""
    recs = corpus.text_records(n, seed, 250, 500)
    redo = list(range(every - 1, n, every))
    marked = set(redo)
    items = [(len(r), corpus.gzip_members(r, [len(r) // 3]) if i in marked else corpus.gzip_member(r))
             for i, r in enumerate(recs)]
    return corpus.gz_file(items), recs, redo


def embedded_redo_file(n=60, every=10, seed=32):
    """(image, records, indices of the records of two members): stored (level 0) members whose data are
    themselves recordio files, so chunk starts inside them find CRC-valid headers that are not on the
    chain and the placement comes from the sequential repair; every `every`-th record has two members.
    k_gz_resize documents a hand-back at the first such record for these files (`st->slow`)."""
    recs = [bytes(r) for r in corpus.embedded_file_records(n, seed)]
    redo = [i for i in range(every - 1, n, every)]
    for i in redo:
        recs[i] = recs[i - 1 if len(recs[i]) < 100 else i]  # a long (embedded-file) record
    marked = set(redo)
    items = [(len(r), corpus.gzip_members(r, [len(r) // 2], level=0) if i in marked else corpus.gzip_member(r, 0))
             for i, r in enumerate(recs)]
    return corpus.gz_file(items), recs, redo
