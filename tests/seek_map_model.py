"""A plain model of the reader's SeekNext map, and the files that pin it.

The map (build_seek_map, csrc/rio_seek.hip) is P, every 0x91 offset of a file, and R, where a SeekNext
walk from that offset ends. The model here is written from MMapReader.SeekNext (mmap_reader.go:58-128),
not from the kernels: from a 0x91 at p the scan's own step is `91 X` -> p + 2, `91 8d Y` -> p + 3, and a
full marker runs a trial ReadNextAt (the oracle's), whose io.EOF / magic / header-CRC class continues at
p + 3 while anything else ends the call there. A marker cut by the file end is io.EOF (the rewind at
:94-97 re-reads from it and :121-124 returns). Ends are resolved right to left, one step per position.

The case families (name -> image) are shared by tests/test_seek_map_host.py, which checks the model
against the oracle's SeekNext and each family against what it declares to contain, and by
tests/test_gpu_seek_map.py, which checks the device's P / R against the model.
"""
import ctypes
import functools
import random

import numpy as np

import corpus
import oracle_py as orc

OTHER = (1 << 63) - 1  # RIO_SEEK_END_OTHER: a trial outside the decoded sequence ends the walk
EOF = OTHER - 1        # RIO_SEEK_END_EOF: the walk runs to the file end
SEG = 4096             # kSegBytes: a wave of k_count91 / k_list91 takes one segment, a lane 64 bytes, a load 16
# a trial's error classes that SeekNext scans on from (mmap_reader.go:108): HeaderChecksumMismatchErr,
# MagicNumberMismatchErr and whatever wraps io.EOF
BENIGN = {1, 2, 3, 4, 22, 6, 7}


_held = [None, None]


def _cbuf(raw: bytes):
    """The oracle's input buffer for `raw`, kept while the same object is asked about again (oracle_py
    copies the image per call, which is most of a call's time on the multi-megabyte files)."""
    if _held[0] is not raw:
        _held[:] = [raw, ctypes.create_string_buffer(raw, len(raw) + 1)]
    return _held[1], len(raw)


def read_next_at(raw: bytes, off):
    """oracle_py.read_next_at (orc_read_next_at on the held buffer): (status, record)."""
    b, n = _cbuf(raw)
    out, ol, nil, d0, d1 = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_int(), ctypes.c_uint64(), ctypes.c_uint64()
    st = orc.lib().orc_read_next_at(b, n, off, ctypes.byref(out), ctypes.byref(ol), ctypes.byref(nil), ctypes.byref(d0),
                                    ctypes.byref(d1))
    rec = None
    if st == 0 and not nil.value:
        rec = ctypes.string_at(out.value, ol.value) if ol.value else b""
    if out.value:
        orc.lib().orc_free(out)
    return st, rec


def seek_next(raw: bytes, off, seek_len=4096):
    """oracle_py.seek_next (orc_seek_next on the held buffer): (status, record offset, record)."""
    b, n = _cbuf(raw)
    ro, out, ol, nil = ctypes.c_uint64(), ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_int()
    st = orc.lib().orc_seek_next(b, n, off, seek_len, ctypes.byref(ro), ctypes.byref(out), ctypes.byref(ol),
                                 ctypes.byref(nil))
    rec = None
    if st == 0 and not nil.value:
        rec = ctypes.string_at(out.value, ol.value) if ol.value else b""
    if out.value:
        orc.lib().orc_free(out)
    return st, ro.value, rec


def disk_index_search(raw: bytes, key: bytes, seek_len=4096):
    """oracle_py.disk_index_search (orc_disk_index_search on the held buffer)."""
    b, n = _cbuf(raw)
    off, vo, cs, found = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int()
    st = orc.lib().orc_disk_index_search(b, n, bytes(key) or b"\0", len(key), seek_len, ctypes.byref(off),
                                         ctypes.byref(found), ctypes.byref(vo), ctypes.byref(cs))
    return st, off.value, bool(found.value), vo.value, cs.value


def _u8(img):
    return np.frombuffer(img, dtype=np.uint8) if isinstance(img, (bytes, bytearray)) else img


def positions(img):
    return np.flatnonzero(_u8(img) == 0x91).astype(np.uint64)


def ends(img, rec_off, with_steps=False):
    """R of the model: per 0x91 position a record number (index into rec_off, the FileReader
    sequence's record offsets), EOF or OTHER. with_steps: also the walk's length in steps."""
    a = _u8(img)
    raw = a.tobytes() if not isinstance(img, bytes) else img
    n = len(raw)
    P = positions(a).astype(np.int64)
    K = P.shape[0]
    rec_at = {int(o): j for j, o in enumerate(rec_off)}
    R = np.zeros(K, dtype=np.uint64)
    steps = np.zeros(K, dtype=np.int64)
    for k in range(K - 1, -1, -1):
        p = int(P[k])
        if p + 1 >= n or (raw[p + 1] == 0x8D and p + 2 >= n):  # a marker cut by the file end
            R[k] = EOF
            continue
        if raw[p + 1] != 0x8D:
            c = p + 2
        elif raw[p + 2] != 0x4C:
            c = p + 3
        else:
            st = read_next_at(raw, p)[0]
            if st not in BENIGN:
                R[k] = rec_at.get(p, OTHER)
                continue
            c = p + 3
        nk = int(np.searchsorted(P, c))
        if nk >= K:  # no 0x91 left: the scan reads to the file end
            R[k] = EOF
            steps[k] = 1
        else:
            R[k] = R[nk]
            steps[k] = steps[nk] + 1
    return (R, steps) if with_steps else R


def oracle_end(img, rec_at, off, seek_len=4096):
    """What the oracle's SeekNext from `off` ends at, in the map's terms."""
    st, ro, _ = seek_next(img, off, seek_len)
    if st == 1:
        return EOF
    assert st != 14, off
    return rec_at.get(ro, OTHER)


# ------------------------------------------------------------------------------------------------
# building blocks
# ------------------------------------------------------------------------------------------------
def filler(n, seed=0):
    """n bytes, none of them 0x91 (nor 0x8d / 0x4c, so that nothing placed in it grows)."""
    a = (np.arange(n, dtype=np.int64) * 7 + seed) % 97 + 0x20  # 0x20 .. 0x80
    a[a == 0x4C] = 0x2E
    return a.astype(np.uint8)


def rec(payload: bytes) -> bytes:
    """An uncompressed v4 record as FileWriter frames it."""
    return corpus.header_v4(len(payload), 0) + bytes(payload)


LIVE = rec(b"abc")  # embedded in a payload: its trial succeeds outside the decoded sequence
_dead_pre = b"\x91\x8d\x4c\x00\x05\x00"
DEAD = _dead_pre + corpus.uvarint(corpus.crc32c(_dead_pre) ^ 0x40)  # a header that fails its CRC
ITEMS = {"lone": b"\x91", "pair": b"\x91\x8d", "dead": DEAD, "live": LIVE}
assert all(v.count(b"\x91") == 1 for v in ITEMS.values())
DELTAS = (-3, -2, -1, 0, 1, 2)


# ------------------------------------------------------------------------------------------------
# boundaries
# ------------------------------------------------------------------------------------------------
B16, B64, B4096, TAIL = 16 * 65, 64 * 33, SEG, 300  # a multiple of 16 only, of 64 only, of 4096; bytes past 3 segments


def boundary_places(delta):
    """Where a boundaries file puts its item: (boundary kind, file offset)."""
    return [(16, B16 + delta), (64, B64 + delta), (4096, B4096 + delta), ("last", 3 * SEG + delta)]


def boundary_file(item, delta):
    """Three segments and a tail of 700-byte records (a walk from the filler soon meets a decoded
    record), the item written into the payloads at its four places."""
    blob = np.frombuffer(ITEMS[item], np.uint8)
    img = np.concatenate([np.frombuffer(corpus.file_header(), np.uint8), filler(3 * SEG + TAIL - 8, seed=len(item) + delta)])
    for _, at in boundary_places(delta):
        img[at:at + blob.shape[0]] = blob
    p, h = 8, corpus.header_v4(700, 0)
    while p < img.shape[0]:
        if img.shape[0] - p < 700 + len(h):  # the last record takes what is left
            h = next(x for n in range(24) if len(x := corpus.header_v4(img.shape[0] - p - n, 0)) == n)
        # no header stands on or next to a placed item
        assert all(at + blob.shape[0] + 8 < p or p + len(h) + 8 < at for _, at in boundary_places(delta)), (item, delta)
        img[p:p + len(h)] = np.frombuffer(h, np.uint8)
        p += len(h) + (700 if h == corpus.header_v4(700, 0) else img.shape[0] - p - len(h))
    assert (img.shape[0] - 1) // SEG == 3  # the last segment starts at 3 * SEG
    return img.tobytes()


def boundaries():
    return {f"bnd_{item}_{d:+d}": boundary_file(item, d) for item in ITEMS for d in DELTAS}


# ------------------------------------------------------------------------------------------------
# tails
# ------------------------------------------------------------------------------------------------
TAILS = (b"\x91", b"\x91\x8d", b"\x91\x8d\x4c", b"\x91\x00")


def tail_file(length, tail):
    """A file of `length` bytes whose last record's payload ends in `tail`."""
    for mid in range(40, 48):
        head = corpus.file_header() + rec(b"first") + rec(filler(mid).tobytes())
        while length - len(head) > 1500:  # decoded records all the way: only the last one's walks run to the file end
            head += rec(filler(700, seed=len(head)).tobytes())
        for hl in range(7, 13):  # the last header's length depends on its payload's (the CRC is a varint)
            pl = length - len(head) - hl
            last = rec(filler(pl - len(tail), seed=length).tobytes() + tail)
            if len(head) + len(last) == length:
                return head + last
    raise AssertionError(length)


def tails():
    out = {f"tail_mod{r}": tail_file(592 + 17 * r, TAILS[r % 4]) for r in range(16)}
    assert sorted(len(v) % 16 for v in out.values()) == list(range(16))
    # every tail also at the quarter's (and the segment's) last byte, and at its first
    out["tail_2seg_exact"] = tail_file(2 * SEG, b"\x91")
    return out


# ------------------------------------------------------------------------------------------------
# segments
# ------------------------------------------------------------------------------------------------
SEGMENT_COUNTS = (1, 3, 4, 5, 1023, 1024, 1025, 1027, 2049)
REC = 65536


def segment_file(nseg):
    """A file of nseg segments of 64 KiB uncompressed records: one 0x91 per segment, its lane, quarter
    and byte rotating, and in each of the three last segments a lane of 64 0x91 bytes. Returns a numpy
    image (headers are written over whatever the placement put where they stand)."""
    want = (nseg - 1) * SEG + 2503
    heads, p = [], 8
    while p < want:  # the layout first: a header does not depend on its payload's bytes
        left = want - p
        h = corpus.header_v4(REC if left > REC + 64 else max(left - 10, 0), 0)
        heads.append((p, h))
        p += len(h) + (REC if left > REC + 64 else max(left - 10, 0))
    total = p  # within a few bytes of `want`: the last header's CRC varint has no fixed length
    img = filler(total, seed=nseg)
    for s in range(nseg):
        at = s * SEG + (s * 7 % 64) * 64 + (s % 4) * 16 + s * 5 % 16
        if at < total:
            img[at] = 0x91
    for s in range(max(nseg - 3, 0), nseg):
        at = s * SEG + ((s * 11 + 5) % 64 if s < nseg - 1 else s % 32 + 1) * 64  # (the last segment is 2.5 KB)
        img[at:min(at + 64, total)] = 0x91
    img[:8] = np.frombuffer(corpus.file_header(), np.uint8)
    for at, h in heads:
        img[at:at + len(h)] = np.frombuffer(h, np.uint8)
    assert (total + SEG - 1) // SEG == nseg
    return img


def segments():
    return {f"seg_{n}": segment_file(n) for n in SEGMENT_COUNTS}


# ------------------------------------------------------------------------------------------------
# chains
# ------------------------------------------------------------------------------------------------
CHAIN_L = (1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025)
CHAIN_GROUPS = {"small": CHAIN_L[:10], "mid": CHAIN_L[10:13], "big": CHAIN_L[13:]}
LONG_RUN = 270_001


def run_file(Ls):
    """Per L a record of 2L and one of 2L + 1 0x91 bytes, each followed by a live record: the run's
    last byte stands right before the next marker, so one parity of the run walks onto that marker
    and the other over it."""
    recs = []
    for L in Ls:
        for n in (2 * L, 2 * L + 1):
            recs += [b"\x91" * n, b"live-%d" % n]
    return corpus.file_header() + b"".join(rec(r) for r in recs)


def train_file(Ls):
    """The same lengths in dead markers: every one is a trial that fails its header CRC."""
    recs = []
    for L in Ls:
        for n in (2 * L, 2 * L + 1):
            recs += [DEAD * n, b"live-%d" % n]
    return corpus.file_header() + b"".join(rec(r) for r in recs)


def long_run_file():
    return corpus.file_header() + rec(b"\x91" * LONG_RUN) + rec(b"def") + rec(b"ghi")


def chains():
    out = {}
    for g, Ls in CHAIN_GROUPS.items():
        out[f"chain_runs_{g}"] = run_file(Ls)
        out[f"chain_trains_{g}"] = train_file(Ls)
    out["chain_long_run"] = long_run_file()
    return out


# ------------------------------------------------------------------------------------------------
# ends: every way a walk ends, and the other file kinds
# ------------------------------------------------------------------------------------------------
def _embedded(last_payload_tail):
    past_end = corpus.header_v4(1 << 20, 0)  # a valid header whose payload would pass the file end
    recs = [b"plain", b"x" + LIVE + b"y", b"x" + past_end + b"y", b"x" + DEAD + b"y",
            b"x\x91\x8d" + LIVE + b"y",  # 91 8d 91: the scan's step passes over the marker behind it
            b"\x91\x91\x8d" + LIVE, b"zz\x91", b"after", b"tail" + last_payload_tail]
    return corpus.file_header() + b"".join(rec(r) for r in recs)


def _text(n, seed):
    return corpus.text_records(n, seed, 20, 400)


def ends_files():
    from recordio import encode_file

    out = {}
    # a header torn after a whole varint (io.EOF: the walk goes on to the file end) and inside one
    # (io.ErrUnexpectedEOF: the walk ends there)
    out["end_embedded_torn_eof"] = _embedded(b"\x91\x8d\x4c\x00\x05")
    out["end_embedded_torn_mid"] = _embedded(b"\x91\x8d\x4c\x00\x85")
    t = _text(12, 3)
    bad_snappy = corpus.uvarint(170) + b"\xf0\x9f" + bytes(range(160))  # 160 bytes where the preamble says 170
    sn = bytes(encode_file([t[0], None, t[1], b"", t[2]], 2))
    sn += corpus.header_v4(160, len(bad_snappy)) + bad_snappy
    sn += bytes(encode_file([t[3], None, b"\x91" * 40 + t[4]], 2))[8:]
    out["end_snappy"] = sn
    gz = [(len(r), corpus.gzip_member(r)) for r in t]
    gz[2] = None
    gz[4] = (0, b"")  # gzip.NewReader on no bytes: io.EOF, a trial the walk passes
    gz[6] = (gz[6][0], gz[6][1][:len(gz[6][1]) // 2])
    gz[9] = None
    out["end_gzip"] = corpus.gz_file(gz)
    lz = [(len(r), orc.lzw_encode(r)) for r in t]
    lz[2] = None
    lz[6] = (lz[6][0], lz[6][1][:-2])
    lz[9] = None
    out["end_lzw"] = corpus.lzw_file(lz)
    marked = [b"a\x91b", None, b"\x91\x8d", b"q" + b"\x91" * 9, b"", b"\x91\x8d\x4c\x00", b"end\x91"]
    out["end_v3"] = corpus.v3_file(marked, 0)
    out["end_v2"] = corpus.legacy_file([r for r in marked if r is not None], 0, 2)
    img = bytearray(encode_file([b"rec-%d\x91" % i for i in range(12)], 0))
    o = orc.file_reader_decode(bytes(img))
    img[o["rec_off"][6] + 3] ^= 0x02  # record 6's header fails its CRC: the FileReader sequence stops there
    out["end_mid_break"] = bytes(img)
    out["end_header_only"] = corpus.file_header()
    out["end_empty"] = b""
    return out


FAMILIES = {"boundaries": boundaries, "tails": tails, "segments": segments, "chains": chains, "ends": ends_files}
LARGE = ("segments", "chain_long_run")  # sampled, not walked from every position


@functools.lru_cache(maxsize=None)
def family(name):
    return FAMILIES[name]()


def all_names():
    """(family, file name) of every file, without building the large ones."""
    fixed = {"segments": [f"seg_{n}" for n in SEGMENT_COUNTS]}
    return [(f, n) for f in FAMILIES for n in (fixed.get(f) or list(family(f)))]


@functools.lru_cache(maxsize=None)
def solved(fam, name):
    """(image bytes, the oracle's record offsets, P, R, steps) of one file; computed once, shared,
    and not to be written to."""
    img = family(fam)[name]
    raw = img.tobytes() if isinstance(img, np.ndarray) else bytes(img)
    if len(raw) < 8:
        return raw, [], np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.int64)
    rec_off = [int(x) for x in orc.file_reader_decode_arrays(_u8(raw))["rec_off"]]
    R, steps = ends(raw, rec_off, with_steps=True)
    return raw, rec_off, positions(raw), R, steps


def sample(fam, name, count=500):
    """The positions (indices into P) the two large families are checked at: every one within 8
    bytes of a 4096-byte boundary, the first and last 8, and `count` seeded ones."""
    raw, _, P, _, _ = solved(fam, name)
    K = P.shape[0]
    near = np.flatnonzero((P.astype(np.int64) + 8) % SEG < 16)
    rng = random.Random(len(raw))
    pick = set(near.tolist()) | set(range(min(8, K))) | set(range(max(K - 8, 0), K))
    pick |= {rng.randrange(K) for _ in range(count)} if K else set()
    return sorted(pick)
