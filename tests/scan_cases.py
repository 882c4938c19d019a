"""Files that put the chunk scan (k_scan_blocks, rio_chunk_scan.hip) and the placement prologue (k_place,
rio_place.hip) at the boundaries of the scan tree, and a plain sequential model of what the scan must find.

At 64-byte chunks every structure of the tree is reachable with small files: a level-1 block is 256 chunks
(16 KiB), level 2 runs in one wave up to 64 blocks (16 384 chunks, 1 MiB) and in tiles of 256 block runs with a
carry beyond that (a second tile from 65 536 chunks, 4 MiB, on).

Host only, numpy only. A `Layout` lays v4 uncompressed records down and keeps a ledger of what it wrote: every
record of the chain, and every position holding the magic bytes 91 8d 4c with two claims about it: whether the
chain reaches it, and whether it frames (a right header CRC and a payload inside the file: find_entry's rule,
rio_frame.h). `finish` searches the image for the magic bytes and insists that the ledger lists exactly those
positions. `model` then works from the ledger alone, never from a composition tree: it follows the chain from
offset 8 in FileReader order and gives, per chunk, where the chain arrives, the speculative entry a walk must
find, the records owned, and the number of chunks the serial repair (slow_path) would walk again.

tests/test_scan_cases_host.py checks every claim made here against the oracle on the CPU;
tests/test_gpu_chunk_scan.py runs the same list on the device under both walks."""
import dataclasses
import functools

import numpy as np

import corpus

CB = 64            # chunk bytes of both framings in these tests (the smallest rio_ctx_create accepts)
BLOCK = 256        # chunks per level-1 block (kScanBlock)
TILE = 256         # block runs per level-2 tile
WAVE_BLOCKS = 64   # level 2 runs in one wave up to this many blocks
HDR = 8            # file header bytes
FILL = 0x61        # payload byte (not 0x91: a payload of it holds no magic)
NONE = -1          # "no position" in the model's arrays
MIN_REC = 11       # the smallest record here: magic 3, nil 1, u 1, c 1, CRC 5 (padded), no payload

N1 = 600                 # level 2 in one wave
N2 = 16384 + 600         # level 2 tiled, one tile (67 blocks): block barriers, identity carry
N3 = 65536 + 600         # two tiles: the second meets a non-identity carry


def cs(c: int) -> int:
    """First byte of chunk c."""
    return HDR + c * CB


def geometry(length: int, cb: int = CB):
    """(n_chunks, n_blocks, n_tiles) of a file of `length` bytes."""
    n_chunks = -(-(length - HDR) // cb) if length > HDR else 0
    n_blocks = -(-n_chunks // BLOCK)
    return n_chunks, n_blocks, -(-n_blocks // TILE)


def level2_path(n_blocks: int) -> str:
    return "one wave" if n_blocks <= WAVE_BLOCKS else "tiled"


# ---- records -------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def header(u: int, nu: int, flip: bool = False) -> bytes:
    """The v4 header of an uncompressed record of u payload bytes: u in nu varint bytes, the CRC padded to five, so
    11 bytes for u < 128 and 12 from u = 128 on. flip: one CRC byte is wrong (bit 6 of the first one: the varint
    keeps its length)."""
    ub = corpus.padded_uvarint(u, nu)
    crc = corpus.crc32c(b"\x91\x8d\x4c\x00" + ub + b"\x00") ^ (0x40 if flip else 0)
    return corpus.header_v4(u, 0, u_bytes=ub, crc_bytes=corpus.padded_uvarint(crc, 5))


def split_total(total: int):
    """(u, nu) of the record of exactly `total` encoded bytes: the shortest size varint that fits (one byte longer
    than canonical for the few totals no canonical header reaches, such as 139)."""
    for nu in range(1, 6):
        u = total - 10 - nu
        if 0 <= u < 1 << (7 * nu):
            return u, nu
    raise ValueError(total)


def rec_total(total: int, fill: int = FILL, flip: bool = False) -> bytes:
    """One record of exactly `total` encoded bytes, its payload one byte value."""
    assert fill != 0x91
    u, nu = split_total(total)
    return header(u, nu, flip) + bytes([fill]) * u


@dataclasses.dataclass
class Ledger:
    length: int
    rec_off: np.ndarray     # starts of the chain's records, in order
    rec_len: np.ndarray     # their encoded bytes
    rec_u: np.ndarray       # their payload (= decoded) bytes
    mag_pos: np.ndarray     # every position of 91 8d 4c, ascending
    mag_chain: np.ndarray   # the chain arrives there
    mag_frames: np.ndarray  # frame_record accepts it
    status: str             # the file's terminal status (a key of conftest.STATUS)
    status_offset: int
    detail: tuple           # (stored CRC, computed CRC) behind HEADER_CRC, else None
    stop: int               # where the chain stops before the file's end (the failing position), or NONE
    event: int              # the position the case is about, or NONE


class Layout:
    """Bytes and ledger together. Records written after the chain has stopped are on no chain: they are listed as
    candidates that frame, nothing more."""

    def __init__(self):
        self.parts = [np.frombuffer(corpus.file_header(4, 0), np.uint8)]
        self.pos = HDR
        self.recs, self.mags = [], []
        self.status, self.status_offset, self.detail, self.stop, self.event = "EOF", None, None, NONE, NONE

    def _put(self, b):
        a = np.frombuffer(b, np.uint8) if isinstance(b, (bytes, bytearray)) else b
        self.parts.append(a)
        self.pos += len(a)

    def _mag(self, pos, chain, frames):
        pos = np.atleast_1d(np.asarray(pos, np.int64))
        self.mags.append((pos, np.full(len(pos), chain), np.full(len(pos), frames)))

    def _records(self, starts, total, u):
        starts = np.atleast_1d(np.asarray(starts, np.int64))
        live = self.stop == NONE
        if live:
            self.recs.append((starts, np.full(len(starts), total, np.int64), np.full(len(starts), u, np.int64)))
        self._mag(starts, live, True)

    def _stop(self, status, detail=None):
        assert self.stop == NONE
        self.stop = self.status_offset = self.event = self.pos
        self.status, self.detail = status, detail

    def fill(self, total: int, n: int):
        """n records of `total` bytes each, one np.tile."""
        if n > 0:
            r = rec_total(total)
            self._records(self.pos + total * np.arange(n, dtype=np.int64), total, split_total(total)[0])
            self._put(np.tile(np.frombuffer(r, np.uint8), n))

    def rec(self, total: int) -> int:
        at = self.pos
        self.fill(total, 1)
        return at

    def to(self, target: int, filler: int = 40):
        """Fillers, then one pad record of the right length, so that the next record starts at `target`."""
        gap = target - self.pos
        assert gap == 0 or gap >= MIN_REC, (self.pos, target)
        if gap:
            n = (gap - MIN_REC) // filler
            self.fill(filler, n)
            self.rec(gap - n * filler)

    def at(self, c: int, how: str, shift: int = 0):
        """The next record starts in chunk c. "first": at cs(c) + shift, as the chunk's first record start.
        "later": a 12-byte record at cs(c) + 3 and the next one at cs(c) + 15 (in chunk 0, where the chain starts at
        its first byte, the 12-byte record is at 8 and the next one at 20)."""
        if how == "first":
            self.to(cs(c) + shift)
        else:
            self.to(cs(c) + (3 if c else 0))
            self.rec(12)
        return self.pos

    def bad_crc(self, total: int):
        """A record whose stored header CRC is wrong: the chain stops at it."""
        u, nu = split_total(total)
        good = corpus.crc32c(header(u, nu)[:5 + nu])
        self._mag(self.pos, True, False)
        self._stop("HEADER_CRC", (good ^ 0x40, good))
        self._put(rec_total(total, flip=True))

    def cut_header(self):
        """The file ends three bytes into a record's header (its magic is whole)."""
        self._mag(self.pos, True, False)
        self._stop("EOF_HEADER")
        self._put(rec_total(40)[:3])

    def cut_payload(self, end: int):
        """A record whose payload is twice what the file holds behind its header: the file ends at `end`."""
        for nu in range(2, 6):
            u = 2 * (end - self.pos - 10 - nu)
            if len(corpus.uvarint(u)) == nu:
                break
        assert u >= 128 and len(corpus.uvarint(u)) == nu
        self._mag(self.pos, True, False)
        self._stop("UNEXPECTED_EOF")
        self._put(header(u, nu))
        self._put(np.full(end - self.pos, FILL, np.uint8))

    def zeros(self, end: int, nonzero: bool):
        """Zeros from here to the file's end at `end`; nonzero: but for one byte near it."""
        self._stop("MAGIC" if nonzero else "EOF_ZERO_TAIL")
        z = np.zeros(end - self.pos, np.uint8)
        if nonzero:
            z[-5] = 1
        self._put(z)

    def span(self, end: int, runs=()):
        """One record from here to `end`. runs: (position, total, count): `count` complete valid records of `total`
        bytes each inside its payload from `position` on: candidates that frame, on no chain."""
        at, total = self.pos, end - self.pos
        u, nu = split_total(total)
        self._records(at, total, u)
        pay = np.full(u, FILL, np.uint8)
        p0 = at + 10 + nu
        for pos, t, n in runs:
            assert p0 <= pos and pos + t * n <= end
            pay[pos - p0:pos - p0 + t * n] = np.tile(np.frombuffer(rec_total(t, 0x62), np.uint8), n)
            self._mag(pos + t * np.arange(n, dtype=np.int64), False, True)
        self._put(header(u, nu))
        self._put(pay)

    def finish(self):
        img = np.concatenate(self.parts)
        assert len(img) == self.pos
        def cat(rows, k, dt):
            return np.concatenate([x[k] for x in rows]).astype(dt) if rows else np.zeros(0, dt)

        mp = cat(self.mags, 0, np.int64)
        order = np.argsort(mp, kind="stable")
        led = Ledger(len(img), cat(self.recs, 0, np.int64), cat(self.recs, 1, np.int64), cat(self.recs, 2, np.int64),
                     mp[order], cat(self.mags, 1, bool)[order], cat(self.mags, 2, bool)[order], self.status,
                     len(img) if self.status_offset is None else self.status_offset, self.detail, self.stop, self.event)
        # the ledger lists every 91 8d 4c of the image, and nothing else
        assert np.array_equal(magic_positions(img), led.mag_pos), "ledger and image disagree on 91 8d 4c"
        assert np.all(np.diff(led.rec_off) == led.rec_len[:-1])
        return img, led


def magic_positions(img: np.ndarray) -> np.ndarray:
    if len(img) < 3:
        return np.zeros(0, np.int64)
    return np.flatnonzero((img[:-2] == 0x91) & (img[1:-1] == 0x8D) & (img[2:] == 0x4C)).astype(np.int64)


def frames_in_image(img: np.ndarray, pos: np.ndarray) -> np.ndarray:
    """Whether each position frames, read from the image (the ledger's claim is checked against this): the v4 header
    parses with the right CRC and the payload of an uncompressed record lies inside the file. One parse per distinct
    16-byte window."""
    padded = np.concatenate([img, np.zeros(16, np.uint8)])
    win = np.ascontiguousarray(padded[pos[:, None] + np.arange(16)])
    half = win.view(np.uint64)  # the windows told apart by a 64-bit mix of their halves, then compared in full
    mix = half[:, 0] * np.uint64(0x9E3779B97F4A7C15) + half[:, 1]
    _, first, inv = np.unique(mix, return_index=True, return_inverse=True)
    uniq, inv = win[first], inv.reshape(-1)
    assert np.array_equal(uniq[inv], win)
    ok, hl, uu = np.zeros(len(uniq), bool), np.zeros(len(uniq), np.int64), np.zeros(len(uniq), np.int64)
    for k, w in enumerate(uniq.tolist()):
        def varint(i):
            v = sh = 0
            while i < 16:
                v |= (w[i] & 0x7F) << sh
                sh += 7
                i += 1
                if w[i - 1] < 0x80:
                    return v, i
            return None, i
        if w[:3] != [0x91, 0x8D, 0x4C]:
            continue
        u, i = varint(4)
        c, j = varint(i) if u is not None else (None, i)
        crc, e = varint(j) if c is not None else (None, j)
        if crc is None or corpus.crc32c(bytes(w[:j])) != crc:
            continue
        ok[k], hl[k], uu[k] = True, e, 0 if w[3] == 1 else u
    return ok[inv] & (pos + hl[inv] + uu[inv] <= len(img))


# ---- the sequential model ------------------------------------------------------------------------------------
def _entries(led: Ledger, n_chunks: int, cb: int) -> list:
    """Per chunk, the speculative entry: the first ledger position in the chunk that frames; chunk 0's is 8."""
    e = [NONE] * n_chunks
    for p in led.mag_pos[led.mag_frames].tolist():
        c = (p - HDR) // cb
        if e[c] == NONE:
            e[c] = p
    if n_chunks:
        e[0] = HDR
    return e


def model(led: Ledger, cb: int = CB) -> dict:
    """What the scan must find, from the ledger alone: one loop over the chunks with the chain position carried along,
    in FileReader order. A chunk is entered when the chain, not yet stopped, arrives at a position before the chunk's
    end. expected_repairs counts the entered chunks whose speculative entry is not that position: exactly the chunks
    slow_path walks again, so the number the device reports whichever path it took. must_be_fast: no repair, and no
    chunk the chain passes through or never reaches holds a candidate that frames (nothing in the file can break the
    composed run). The arrays give each chunk's arrival, entry and placement."""
    n_chunks = geometry(led.length, cb)[0]
    e = _entries(led, n_chunks, cb)
    off, ln, u = led.rec_off.tolist(), led.rec_len.tolist(), led.rec_u.tolist()
    cur, i, idx, nbytes, repairs, stopped, stray = HDR, 0, 0, 0, 0, False, False
    arrive, owned, base_idx, base_bytes = [], [], [], []
    for c in range(n_chunks):
        ce = min(cs(c + 1), led.length)
        base_idx.append(idx)
        base_bytes.append(nbytes)
        own, y = 0, NONE
        if not stopped and cur < ce:
            y = cur
            repairs += e[c] != y
            while cur < ce:
                if cur == led.stop:
                    stopped = True
                    break
                assert off[i] == cur
                own, idx, nbytes, cur, i = own + 1, idx + 1, nbytes + u[i], cur + ln[i], i + 1
        elif e[c] != NONE:
            stray = True
        arrive.append(y)
        owned.append(own)
    assert i == len(off) and (stopped or cur == led.length)
    a = lambda x: np.array(x, np.int64)  # noqa: E731
    return dict(n_chunks=n_chunks, expected_repairs=int(repairs), must_be_fast=repairs == 0 and not stray,
                arrive=a(arrive), entry=a(e), owned=a(owned), base_idx=a(base_idx), base_bytes=a(base_bytes))


# ---- the cases -----------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    group: str              # the test id it runs under: tree, position and kind
    make: tuple             # (builder name, arguments)
    n_chunks: int           # the chunk count the case is named for
    repairs: tuple = None   # the engineered ("eq" | "ge", k) of expected_repairs; None: the model alone says
    fast: bool = None       # must_be_fast as engineered; None: not claimed
    cstar: int = None       # the chunk of the event
    how: str = None         # "first": the event is its chunk's first record start; "later": it is not


def _end(n: int, last: int = CB) -> int:
    """File length for n chunks, the last one holding `last` bytes."""
    return cs(n - 1) + last


def make_shape(n, filler, last):
    L = Layout()
    if n == 1 and last == 1:
        # no record fits one byte: the one shape that cannot be a clean file. The byte is a whole varint that is not
        # the magic, and nothing follows it: FileReader's zero-tail rule (file_reader.go:76-91) calls that a clean end
        L._stop("EOF_ZERO_TAIL")
        L._put(bytes([FILL]))
    else:
        L.to(_end(n, last), filler)
    return L.finish()


def _tail(L, n):
    L.to(_end(n))


def make_crc(n, c, variant):
    """variant: "later" | "at8" | "first0" | "first5" | "alone0" | "alone5"."""
    L, end = Layout(), _end(n)
    if variant == "later":
        L.at(c, "later")
        # in the tree's last chunk the record runs to the file's end: a valid record behind it would frame off the chain
        # in a chunk the chain enters
        L.bad_crc(20 if c < n - 1 else end - L.pos)
    elif variant == "at8":
        L.bad_crc(20)
    elif variant.startswith("first"):
        L.at(c, "first", int(variant[5:]))
        L.bad_crc(20)
        L.rec(20)  # the chunk's other record: it frames, so it is the walk's speculative entry
    else:
        L.at(c, "first", int(variant[5:]))
        L.bad_crc(min(80, end - L.pos))  # ends in the next chunk (or with the file): nothing else starts in this one
    _tail(L, n)
    return L.finish()


def make_cut(n, c, what, variant):
    """what: "header" (the file ends in chunk c) | "payload" (the file keeps the tree's length)."""
    L = Layout()
    L.at(c, "later") if variant == "later" else L.at(c, "first", int(variant[5:]))
    if what == "header":
        L.cut_header()
    else:
        L.cut_payload(max(_end(n), cs(c + 3)))
    return L.finish()


def zero_end(n, c):
    """Zero tails reach the tree's end, and cross at least one block boundary: 300 chunks at the least."""
    return max(_end(n), _end(c + 301))


def make_zero(n, c, variant, nonzero):
    L = Layout()
    L.at(c, "later") if variant == "later" else L.at(c, "first")
    if variant == "later":
        L.rec(20)  # the zeros begin where this record ends, in the middle of the chunk
    L.zeros(zero_end(n, c), nonzero)
    return L.finish()


def make_false_on_chain(n, c):
    L = Layout()
    L.to(cs(c) - 10)
    # 50 bytes from cs - 10: the payload is [cs + 1, cs + 40) and holds a whole 20-byte record at cs + 2
    L.span(cs(c) + 40, runs=[(cs(c) + 2, 20, 1)])
    L.event = cs(c) + 40
    _tail(L, n)
    return L.finish()


# spans: (first chunk, chunk of the next record's start, file chunks)
SPAN_A = (200, 768, 900)                                # blocks 1 and 2 own nothing; chunk 768 opens block 3
SPAN_B = (100, 100 + 16384 + 300, 100 + 16384 + 600)    # 64 whole blocks are passed through
SPAN_C = (65000, 65000 + 65536 + 600, 65000 + 65536 + 900)  # the second tile's block runs all have key kNone
RUNS_A = [(cs(512), 32, 3), (cs(254) + 10, 40, 6)]     # at a block's first byte; across the block boundary at 256
RUNS_C = [(cs(66048), 32, 3), (cs(66302) + 10, 40, 6), (cs(65534) + 10, 40, 6)]  # ...; across the tile boundary at 65536


def make_span(first, nxt, n, shift, runs=()):
    """nxt None: the span is the file's last record and ends with chunk n - 1."""
    L = Layout()
    L.to(cs(first) + 20)
    if nxt is None:
        L.span(_end(n), runs)
    else:
        L.span(cs(nxt) + shift, runs)
        L.event = L.pos
        _tail(L, n)
    return L.finish()


def make_one_record(n, behind):
    L = Layout()
    L.span(_end(n))
    if behind:
        L.rec(behind)
    return L.finish()


SHAPE_N = (1, 2, 255, 256, 257, 512, 513, 16383, 16384, 16385, 65535, 65536, 65537, 65793, 131073)
TREES = {"N1": (N1, (0, 255, 256, 599)),
         "N2": (N2, (16383, 16384, 16639, 16640)),
         "N3": (N3, (0, 1, 255, 256, 16383, 16384, 65535, 65536, N3 - 1))}
KINDS = ("crc_later", "crc_first", "crc_alone", "cut_header", "cut_payload", "zero_tail", "false_on_chain")


def _first_shifts(c):
    # a record cannot start 5 bytes into chunk 0: the chain starts at its first byte and no record is that short
    return (0, 5) if c else (0,)


def _cases():
    out = []

    def add(id, group, make, n_chunks, **kw):
        out.append(Case(id, group, make, n_chunks, **kw))

    for n in SHAPE_N:
        for filler in ((32, 40, 80) if n <= 16385 or n == 65537 else (40,)):
            for last in (CB, 1):
                clean = not (n == 1 and last == 1)
                add(f"shape-N{n}-f{filler}-last{last}", f"N{n}", ("make_shape", (n, filler, last)), n,
                    repairs=("eq", 0), fast=True if clean else None)
    for tree, (n, positions) in TREES.items():
        for c in positions:
            g = lambda kind: f"{tree}-c{c}-{kind}"  # noqa: E731
            add(f"{g('crc_later')}", g("crc_later"), ("make_crc", (n, c, "later")), n, repairs=("eq", 0), cstar=c,
                how="later")
            if c == 0:
                add(f"{g('crc_later')}-at8", g("crc_later"), ("make_crc", (n, c, "at8")), n, repairs=("eq", 0), cstar=c,
                    how="first")
            for s in _first_shifts(c):
                # chunk 0's entry is forced to 8, so a wrong CRC there is no repair
                rp = ("ge", 1) if c else ("eq", 0)
                add(f"{g('crc_first')}-at{s}", g("crc_first"), ("make_crc", (n, c, f"first{s}")), n, repairs=rp, cstar=c,
                    how="first")
                add(f"{g('crc_alone')}-at{s}", g("crc_alone"), ("make_crc", (n, c, f"alone{s}")), n, repairs=rp, cstar=c,
                    how="first")
            for what in ("header", "payload"):
                for v in [f"first{s}" for s in _first_shifts(c)] + ["later"]:
                    nc = c + 1 if what == "header" else max(n, c + 3)
                    add(f"{g('cut_' + what)}-{v}", g("cut_" + what), ("make_cut", (n, c, what, v)), nc, cstar=c,
                        how="later" if v == "later" else "first")
            for v in ("later", "first"):
                for nz in (False, True):
                    add(f"{g('zero_tail')}-{v}{'-nonzero' if nz else ''}", g("zero_tail"), ("make_zero", (n, c, v, nz)),
                        geometry(zero_end(n, c))[0], cstar=c, how=v)
            if c:  # nothing precedes chunk 0, and its entry is forced: no false entry can be met there
                add(g("false_on_chain"), g("false_on_chain"), ("make_false_on_chain", (n, c)), n, repairs=("eq", 1),
                    cstar=c, how="first")
    for name, (first, nxt, n) in (("A", SPAN_A), ("B", SPAN_B), ("C", SPAN_C)):
        for shift in ((0, 1, 63) if name == "A" else (7,)):
            add(f"span{name}-next-at-c{nxt}+{shift}", f"span{name}", ("make_span", (first, nxt, n, shift)), n,
                repairs=("eq", 0), fast=True, cstar=nxt, how="first")
    add("spanA-ends-the-file-with-c767", "spanA", ("make_span", (200, None, 768, 0)), 768, repairs=("eq", 0), fast=True)
    add("one-record-of-65537-chunks", "one-record", ("make_one_record", (65537, 0)), 65537, repairs=("eq", 0), fast=True)
    add("one-record-of-65537-chunks-and-20-bytes", "one-record", ("make_one_record", (65537, 20)), 65538, repairs=("eq", 0),
        fast=True)
    add("spanA-false-entries", "span_with_false_entries", ("make_span", SPAN_A + (0, tuple(RUNS_A))), SPAN_A[2],
        repairs=("eq", 0), fast=False, cstar=SPAN_A[1], how="first")
    add("spanC-false-entries", "span_with_false_entries", ("make_span", SPAN_C + (7, tuple(RUNS_C))), SPAN_C[2],
        repairs=("eq", 0), fast=False, cstar=SPAN_C[1], how="first")
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
GROUPS = {}
for _c in CASES:
    GROUPS.setdefault(_c.group, []).append(_c)

# one context decodes these in turn: larger and smaller files alternate, fast and repaired ones too
ONE_CONTEXT = ("shape-N65537-f40-last64", "shape-N1-f40-last64", "N3-c65536-crc_first-at0", "shape-N257-f40-last64",
               "spanC-next-at-c131136+7", "shape-N16385-f40-last64", "N1-c255-false_on_chain", "shape-N2-f40-last64")
assert all(i in BY_ID for i in ONE_CONTEXT)


@functools.lru_cache(maxsize=24)
def built(case_id: str):
    """(image, ledger, model) of a case; the arrays are shared and must stay unchanged."""
    name, args = BY_ID[case_id].make
    img, led = globals()[name](*args)
    img.setflags(write=False)
    return img, led, model(led)
