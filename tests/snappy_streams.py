"""Snappy blocks, records and files built by hand for the lane decoder's tests.

Three layers, none of which decodes anything:

  * elements (`lit`, `copy`, `copy4`) and `Stream`, a block built element by element that keeps its own
    decoded bytes;
  * FORMS, a named table of records: every shape of record that the lane decoder's record switch, far
    history, descriptor fetch and error path treat differently, valid and invalid. A form is a
    function of a random generator returning (payload, decoded or None, valid);
  * `tile`, a file of any number of records in which every ordered pair of forms is adjacent at every
    position of a lane's record range, and CASES, the files the lane-stream tests decode (the host
    test proves from tests/lane_split.py that they reach what the GPU test says they reach).
"""
import math
import random

import numpy as np

import corpus

K_FAR_OFF = 232  # kFarOff, csrc/rio_snappy.hip: copies reaching further back read the output arena


def lit(b: bytes, tag=None) -> bytes:
    """A literal in its shortest length form, or with the 3- / 4-byte length (tag 62 / 63)."""
    n = len(b) - 1
    if tag is not None:
        assert tag in (62, 63)
        return bytes([tag << 2]) + n.to_bytes(tag - 59, "little") + b
    if n < 60:
        return bytes([n << 2]) + b
    if n < 256:
        return bytes([60 << 2, n]) + b
    return bytes([61 << 2, n & 0xFF, n >> 8]) + b


def copy(off: int, ln: int) -> bytes:
    if 4 <= ln <= 11 and off < 2048:
        return bytes([1 | ((ln - 4) << 2) | ((off >> 8) << 5), off & 0xFF])
    if off < 65536:
        return bytes([2 | ((ln - 1) << 2), off & 0xFF, off >> 8])
    return copy4(off, ln)


def copy2(off: int, ln: int) -> bytes:
    return bytes([2 | ((ln - 1) << 2), off & 0xFF, off >> 8])


def copy4(off: int, ln: int) -> bytes:
    """Copy with a 4-byte offset (tag 3), whatever the offset's size."""
    return bytes([3 | ((ln - 1) << 2)]) + off.to_bytes(4, "little")


class Stream:
    """A snappy block built element by element, with the decoded bytes kept to size copies."""

    def __init__(self):
        self.els = bytearray()
        self.out = bytearray()
        self.max_off = 0  # the largest copy offset so far

    def literal(self, b: bytes, tag=None):
        self.els += lit(b, tag)
        self.out += b

    def _copied(self, off, ln):
        self.max_off = max(self.max_off, off)
        for _ in range(ln):
            self.out.append(self.out[-off])

    def copy(self, off: int, ln: int):
        assert 1 <= off <= len(self.out) and 1 <= ln <= 64
        self.els += copy(off, ln)
        self._copied(off, ln)

    def copy4(self, off: int, ln: int):
        assert 1 <= off <= len(self.out) and 1 <= ln <= 64
        self.els += copy4(off, ln)
        self._copied(off, ln)

    def payload(self) -> bytes:
        return corpus.uvarint(len(self.out)) + bytes(self.els)


def file_of(streams) -> bytes:
    img = bytearray(corpus.file_header(4, 2))
    for st in streams:
        pay = st.payload()
        img += corpus.header_v4(len(st.out), len(pay)) + pay
    return bytes(img)


def frame(payload) -> bytes:
    """A record behind a valid v4 header whose lengths are the payload's own: u is the block's
    preamble, c its length. `payload` None: a nil record as the writer frames it (u = 0, c = 1, the
    length of an empty block, and no payload bytes)."""
    if payload is None:
        return corpus.header_v4(0, 1, nil=True)
    u, shift = 0, 0
    for x in payload:  # the preamble, as written (every form's is complete)
        u |= (x & 0x7F) << shift
        shift += 7
        if x < 0x80:
            break
    return corpus.header_v4(u, len(payload)) + payload


def _bytes(rng, n) -> bytes:
    return bytes(rng.randrange(256) for _ in range(n))


# ------------------------------------------------------------------------------------------------
# record forms
# ------------------------------------------------------------------------------------------------
FORMS = {}           # name -> function(rng) -> (payload, or None for a nil record; decoded or None; valid)
FAR_FORMS = set()    # forms with a copy of offset > K_FAR_OFF
LIGHT_FORMS = set()  # valid forms of a few bytes: what a tiling repeats to keep its mean record small
EDGE_LENS = (1, 5, 16, 17, 64)


def _valid_form(name, far=False, light=False):
    def reg(fn):
        def build(rng):
            st = fn(rng)
            assert (st.max_off > K_FAR_OFF) == far, name
            return st.payload(), bytes(st.out), True

        FORMS[name] = build
        if far:
            FAR_FORMS.add(name)
        if light:
            LIGHT_FORMS.add(name)
        return fn

    return reg


def _raw_form(fn):
    FORMS[fn.__name__] = fn
    return fn


@_valid_form("one_byte", light=True)
def one_byte(rng):
    st = Stream()
    st.literal(_bytes(rng, 1))
    return st


@_raw_form
def empty(rng):
    """Preamble 0 and no element: a record of no bytes that is not nil."""
    return b"\x00", b"", True


@_raw_form
def nil(rng):
    return None, None, True


LIGHT_FORMS.update(("empty", "nil"))


@_valid_form("two_piece", light=True)
def two_piece(rng):
    """Over before the decoder's pipeline depth (kD = 4 steps) has passed."""
    st = Stream()
    st.literal(_bytes(rng, 3))
    st.copy(1, 5)
    return st


@_valid_form("overlap")
def overlap(rng):
    """Copies of every offset 1..16, the lengths around one 16-byte piece: a piece that covers its
    whole offset doubles it (`eff`). A record takes two lengths per offset; three records with
    consecutive `rng` draws of the start take all six."""
    lens = (1, 4, 15, 16, 17, 64)
    st = Stream()
    st.literal(_bytes(rng, rng.randrange(16, 21)))
    k = rng.randrange(6)
    for off in range(1, 17):
        st.copy(off, lens[(off + k) % 6])
        st.copy(off, lens[(off + k + 3) % 6])
    return st


@_valid_form("lit_forms")
def lit_forms(rng):
    """Every literal-length form: the tag alone (60 bytes), one length byte (61, 256), two (257),
    and the three- and four-byte lengths (tags 62 and 63) on a 5-byte literal; a copy after each."""
    st = Stream()
    for n, tag in ((60, None), (61, None), (256, None), (257, None), (5, 62), (5, 63)):
        st.literal(_bytes(rng, n), tag)
        st.copy(rng.randrange(1, min(len(st.out), 200) + 1), rng.choice((4, 5, 16, 17, 64)))
    return st


@_valid_form("copy4", light=True)
def copy4_small(rng):
    """A copy with the 4-byte offset form (tag 3) and a small offset."""
    st = Stream()
    st.literal(_bytes(rng, 4))
    st.copy4(2, 7)
    return st


def _edge(rng, offsets, last_far=False) -> Stream:
    """A 260 to 300 byte literal, then a copy at each offset (None: the bytes produced, the record's
    byte 0), each behind a 1 to 3 byte literal so that the destination alignment varies."""
    st = Stream()
    st.literal(_bytes(rng, rng.randrange(260, 301)))
    for off in offsets:
        st.literal(_bytes(rng, rng.randrange(1, 4)))
        st.copy(len(st.out) if off is None else off, rng.choice(EDGE_LENS))
    if last_far:
        st.copy(rng.randrange(K_FAR_OFF + 1, len(st.out) + 1), 64)
    return st


@_valid_form("ring_edge")
def ring_edge(rng):
    """The longest copies the LDS history serves."""
    return _edge(rng, (K_FAR_OFF - 1, K_FAR_OFF, K_FAR_OFF - 1, K_FAR_OFF, K_FAR_OFF))


@_valid_form("far_edge", far=True)
def far_edge(rng):
    """Both sides of the ring / far boundary, and the record's first byte."""
    return _edge(rng, (K_FAR_OFF - 1, K_FAR_OFF, K_FAR_OFF + 1, K_FAR_OFF + 2, None))


@_valid_form("ends_far", far=True)
def ends_far(rng):
    """As far_edge, but the record's last pieces are all far copies: the next record's descriptor
    fetch, which shares the far load's slot, has to wait for the step after them."""
    return _edge(rng, (K_FAR_OFF - 1, K_FAR_OFF, K_FAR_OFF + 1, K_FAR_OFF + 2, None), last_far=True)


def far_from_start_stream(rng, copies=60) -> Stream:
    """Far copies whose source is the record's byte 0, 1 or 2, at every destination alignment: as
    record 0 of a file, 16 bytes from q - r would start below the arena."""
    st = Stream()
    st.literal(_bytes(rng, 250))
    for _ in range(copies):
        st.literal(_bytes(rng, rng.randrange(1, 4)))  # move d & 3
        q = rng.randrange(3)
        st.copy(len(st.out) - q, rng.choice([4, 5, 11, 16, 17, 33, 64]))
    return st


@_valid_form("far_from_start", far=True)
def far_from_start(rng):
    return far_from_start_stream(rng, copies=12)


def _invalid(preamble: int, els: bytes):
    return corpus.uvarint(preamble) + els, None, False


@_raw_form
def copy_first(rng):
    """The first element is a copy of offset 1: behind another record of the lane, the byte it names
    is that record's last."""
    return _invalid(5, copy(1, 5))


@_raw_form
def reach_back(rng):
    """A copy of offset produced + 1: one byte before the record's first."""
    return _invalid(12, lit(_bytes(rng, 8)) + copy(9, 4))


@_raw_form
def off0(rng):
    return _invalid(8, lit(_bytes(rng, 4)) + copy2(0, 4))


@_raw_form
def lit_past_stream(rng):
    """A literal of 10 bytes with 4 bytes left in the stream."""
    return _invalid(10, bytes([9 << 2]) + _bytes(rng, 4))


@_raw_form
def cut_header(rng):
    """The stream ends inside a copy's offset."""
    return _invalid(8, lit(_bytes(rng, 4)) + copy2(2, 4)[:2])


@_raw_form
def cut_lit_len(rng):
    """The stream ends inside a literal's two-byte length."""
    return _invalid(14, lit(_bytes(rng, 4)) + bytes([61 << 2, 9]))


@_raw_form
def short_of_preamble(rng):
    return _invalid(9, lit(_bytes(rng, 6)))


@_raw_form
def long_of_preamble(rng):
    """The last copy would produce 12 bytes where the preamble says 9."""
    return _invalid(9, lit(_bytes(rng, 4)) + copy(1, 8))


VALID = ("far_from_start", "one_byte", "empty", "nil", "two_piece", "overlap", "lit_forms", "copy4", "ring_edge",
         "far_edge", "ends_far")
INVALID = ("copy_first", "reach_back", "off0", "lit_past_stream", "cut_header", "cut_lit_len", "short_of_preamble",
           "long_of_preamble")
ALL = VALID + INVALID
assert set(ALL) == set(FORMS) and LIGHT_FORMS <= set(VALID) and FAR_FORMS <= set(VALID)


def edge_matrix(seed=0):
    """The ring / far boundary in full, one record per case: a copy of every offset 225..240 at every
    destination alignment d & 3 and every length of EDGE_LENS, and after it a short literal and the
    same copy again (its source now holds the first copy's bytes). 320 streams."""
    rng = random.Random(seed)
    out = []
    for off in range(225, 241):
        for r in range(4):
            for ln in EDGE_LENS:
                st = Stream()
                st.literal(_bytes(rng, rng.randrange(260, 301)))
                st.literal(_bytes(rng, (r - len(st.out) - 1) % 4 + 1))
                assert len(st.out) % 4 == r
                st.copy(off, ln)
                st.literal(_bytes(rng, 2))
                st.copy(off, ln)
                out.append(st)
    return out


# ------------------------------------------------------------------------------------------------
# tiled files
# ------------------------------------------------------------------------------------------------
VARIANTS = 3        # framed records per form: a file is joined from a pool of len(forms) * VARIANTS
RPLS = (2, 3, 5)    # records per lane under test: a unit's length is coprime to each


class Tiled:
    """A tiled file: `image` (numpy uint8), `names` (the forms), and per record `seq` (index into
    names), `valid` and `far` (the record holds a copy of offset > K_FAR_OFF)."""

    def __init__(self, image, names, seq):
        self.image, self.names, self.seq = image, names, seq
        self.n = len(seq)
        self.valid = np.array([nm in VALID for nm in names])[seq]
        self.far = np.array([nm in FAR_FORMS for nm in names])[seq]
        self.n_invalid = int(self.n - self.valid.sum())


def _unit(names, main, light_reps, pool):
    """One unit of a tiling as (form index per record, the framed records): for every f, for every g
    of `main`, f then g; the same over the light forms `light_reps` times; then light records up to a
    record count coprime to every RPLS and an odd byte length, so that repeats of the unit put every
    pair at every position of a lane and every record at every offset mod 16."""
    light = [f for f in main if f in LIGHT_FORMS]
    order = [x for f in main for g in main for x in (f, g)]
    order += [x for f in light for g in light for x in (f, g)] * light_reps
    used = {f: 0 for f in main}
    recs = []
    for f in order:
        used[f] += 1
        recs.append(pool[f][used[f] % VARIANTS])

    def padded():
        size = sum(len(r) for r in recs)
        for m in range(64):
            if math.gcd(len(order) + m, math.prod(RPLS)) != 1:
                continue
            if m == 0:
                if size % 2:
                    return [], []
                continue
            # m - 1 records of one light form and one of any: whichever makes the byte length odd
            for a in light:
                for b in light:
                    if (size + (m - 1) * len(pool[a][0]) + len(pool[b][0])) % 2:
                        return [a] * (m - 1) + [b], [pool[a][0]] * (m - 1) + [pool[b][0]]
        raise AssertionError("no padding gives a unit of the wanted length")

    pad_forms, pad_recs = padded()
    idx = np.array([names.index(f) for f in order + pad_forms], dtype=np.int16)
    return idx, recs + pad_recs


def tile(forms, n, seed, light=10, max_full=None) -> Tiled:
    """A Snappy v4 file of n records tiled from `forms` (a tuple of names).

    The file repeats a unit: a pair-complete sequence over the forms (every ordered pair adjacent),
    then `light` pair-complete sequences over the light forms alone, which bring the mean record
    down. With `max_full`, only the first max_full units hold the invalid forms; the later ones are
    units over the valid forms, so that the number of failing lanes stays small. Every form is framed
    VARIANTS times and the file is joined from those records: a v4 header holds nothing that depends
    on the record's position."""
    rng = random.Random(seed)
    names = list(forms)
    pool = {f: [frame(FORMS[f](rng)[0]) for _ in range(VARIANTS)] for f in names}
    valid_names = [f for f in names if f in VALID]
    full = _unit(names, names, light, pool)
    rest = full if len(valid_names) == len(names) or max_full is None else _unit(names, valid_names, light, pool)
    full = full[0], full[1], b"".join(full[1])
    rest = rest[0], rest[1], b"".join(rest[1])
    seqs, parts, left, u = [], [corpus.file_header(4, 2)], n, 0
    while left > 0:
        idx, recs, raw = full if max_full is None or u < max_full else rest
        if len(idx) <= left:
            parts.append(raw)
        else:  # the last, partial unit
            idx = idx[:left]
            parts += recs[:left]
        seqs.append(idx)
        left -= len(idx)
        u += 1
    image = np.frombuffer(b"".join(parts), dtype=np.uint8)
    return Tiled(image, names, np.concatenate(seqs))


# ------------------------------------------------------------------------------------------------
# the files of the lane-stream tests: name -> (records per lane the case is to reach, tile() arguments
# of its lane-decoder files in batch order). Records per lane are rpl of k_snappy_pipe_batch, or rpc of
# k_snappy_pipe for the two "single_..." cases. tests/test_snappy_streams_host.py checks every line of this table
# against tests/lane_split.py; tests/test_gpu_snappy_lane_stream.py decodes the files.
# ------------------------------------------------------------------------------------------------
CASES = {
    # just over 131 072, 262 144 and 524 288 records, split unevenly, the first file no multiple of 64 * rpl
    "rpl2": (2, [(VALID, 70_001, 11), (VALID, 40_000, 12), (VALID, 21_100, 13)]),
    "rpl3": (3, [(VALID, 140_003, 21), (VALID, 80_000, 22), (VALID, 42_200, 23)]),
    "rpl5": (5, [(VALID, 280_001, 31), (VALID, 160_000, 32), (VALID, 84_400, 33)]),
    # N = 130 975: rpl starts at 1, needs 2032 + 30 = 2062 waves of the 2048, and becomes 2
    "need": (2, [(VALID, 65, 100 + k) for k in range(15)] + [(VALID, 130_000, 41)]),
    # invalid forms in the first three units only: at most 1024 failing lanes per file
    "listed": (2, [(ALL, 100_001, 51, 60, 3), (ALL, 31_101, 52, 60, 3)]),
    # invalid forms in every unit: the list of failing lanes overflows
    "overflow": (2, [(ALL, 100_001, 61, 60), (ALL, 31_101, 62, 60)]),
    # one file through k_snappy_pipe, two records per lane; its failing lanes listed (every other lane's
    # bytes and verdicts are then the lane decoder's own: finish_file goes over the listed lanes only) ...
    "single_rpc2": (2, [(ALL, 2_097_152 + 4097, 71, 60, 3)]),
    # ... and overflowing
    "single_rpc2_overflow": (2, [(ALL, 2_097_152 + 4097, 72, 60)]),
}
FAIL_LANES = 1024  # kFailLanes, csrc/rio_device.h


def case_tiles(name):
    return [tile(*args) for args in CASES[name][1]]
