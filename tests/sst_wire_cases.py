"""Wire-format case families for the SSTable parsers (device: csrc/rio_pb.h's pb_index_entry_t and
pb_data_entry_t over pb_varint_t / pb_skip_t, checker: oracle/rio_oracle.c, host mirror: sstables/proto.py)
and a plain model of what proto.Unmarshal makes of each record.

The model restates the rules the parsers' comments cite (protowire.ConsumeVarint, ConsumeFieldValue,
proto.Unmarshal's last-wins and unknown-field behaviour) and shares no code with the three sides it judges:
  a varint has at most 10 bytes and the 10th is at most 1; non-minimal forms are fine
  a field number is 1 .. 2^29-1; wire types 6 and 7 and an end-group tag without its start are errors
  a length, a fixed32 or a fixed64 must fit in what is left of the record
  IndexEntry {key = 1 bytes, valueOffset = 2 varint, checksum = 3 varint}, DataEntry {value = 1 bytes}:
  the last occurrence of a field wins, a known number with another wire type and every other number are skipped
  a group is skipped to its matching end tag; the project allows 16 open groups (a documented choice)

Every family is a list of (name, record bytes). tests/test_sst_wire_cases.py holds model, oracle and mirror
against each other on the CPU; tests/test_gpu_sst_wire.py runs the device parsers at their four call sites."""
import random

from wal_model import field, group, nested_groups

BAD = "BAD"  # data_entry_model's answer for a malformed record (None is Go's nil value)
U64 = (1 << 64) - 1
MAX_FIELD = (1 << 29) - 1
MAX_GROUPS = 16


# ---- the model -------------------------------------------------------------------------------------------
class _Malformed(Exception):
    pass


def _uvarint(b, p):
    v = 0
    for i in range(10):
        if p >= len(b):
            raise _Malformed("varint runs off the record")
        c = b[p]
        p += 1
        if i == 9 and c > 1:
            raise _Malformed("varint above 64 bits")
        v |= (c & 0x7F) << (7 * i)
        if not c & 0x80:
            return v, p
    raise _Malformed("varint longer than 10 bytes")


def _tag(b, p):
    t, p = _uvarint(b, p)
    num, wt = t >> 3, t & 7
    if not 1 <= num <= MAX_FIELD:
        raise _Malformed("field number")
    return num, wt, p


def _value(b, p, num, wt, open_groups=0):
    """-> (payload, position after it) of one field value; payload is the int of a varint, the bytes of a
    length-delimited field, None for everything that is only ever skipped."""
    if wt == 0:
        return _uvarint(b, p)
    if wt == 2:
        n, p = _uvarint(b, p)
        if n > len(b) - p:
            raise _Malformed("length runs off the record")
        return bytes(b[p:p + n]), p + n
    if wt in (1, 5):
        w = 8 if wt == 1 else 4
        if len(b) - p < w:
            raise _Malformed("fixed runs off the record")
        return None, p + w
    if wt == 3:
        if open_groups == MAX_GROUPS:
            raise _Malformed("more than 16 open groups")
        while True:
            n2, w2, p = _tag(b, p)
            if w2 == 4:
                if n2 != num:
                    raise _Malformed("end tag of another group")
                return None, p
            _, p = _value(b, p, n2, w2, open_groups + 1)
    raise _Malformed("wire type %d" % wt)  # 4 without a start, 6, 7


def _fields(rec):
    b, p = bytes(rec), 0
    while p < len(b):
        num, wt, p = _tag(b, p)
        v, p = _value(b, p, num, wt)
        yield num, wt, v


def index_entry_model(rec):
    """-> (key, valueOffset, checksum) of one IndexEntry record, None for a malformed one."""
    key, vo, cs = b"", 0, 0
    try:
        for num, wt, v in _fields(rec):
            if num == 1 and wt == 2:
                key = v
            elif num == 2 and wt == 0:
                vo = v
            elif num == 3 and wt == 0:
                cs = v
    except _Malformed:
        return None
    return key, vo, cs


def data_entry_model(rec):
    """-> the value of one DataEntry record: bytes, None when field 1 is absent (nil), BAD when malformed."""
    value = None
    try:
        for num, wt, v in _fields(rec):
            if num == 1 and wt == 2:
                value = v
    except _Malformed:
        return BAD
    return value


# ---- building blocks -------------------------------------------------------------------------------------
def uv(v, width=0):
    """Varint of v; width > 0 pads it to that many bytes with continuation bits (a non-minimal form)."""
    out = bytearray()
    while v >= 0x80 or len(out) + 1 < width:
        out.append(v & 0x7F | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def tag(num, wt):
    return uv(num << 3 | wt)


K = field(1, b"k")
VO = field(2, 7, 0)
CS = field(3, 9, 0)
EDGE_VALUES = (0, 127, 128, (1 << 32) - 1, 1 << 32, 1 << 63, U64)
# eight bytes that read as fields 2 and 3 when a skip stops four bytes early
F64 = b"\x6b\x6c\x6d\x6e" + field(2, 5, 0) + field(3, 6, 0)
F32 = field(2, 5, 0) + field(3, 6, 0)


def _varints():
    out = []
    for v in EDGE_VALUES:
        out.append(("valueOffset=%#x" % v, field(2, v, 0)))
        out.append(("checksum=%#x" % v, field(3, v, 0)))
        out.append(("key,valueOffset=%#x,checksum=%#x" % (v, v ^ U64), K + field(2, v, 0) + field(3, v ^ U64, 0)))
    out += [
        ("valueOffset 80 00", b"\x10\x80\x00"),
        ("valueOffset nine 80 then 00", b"\x10" + b"\x80" * 9 + b"\x00"),
        ("checksum 5 in three bytes", b"\x18" + uv(5, 3) + K),
        ("length of the key in two bytes", b"\x0a" + uv(1, 2) + b"k" + VO),
        ("10th byte 1", b"\x18" + b"\xff" * 9 + b"\x01"),
        ("10th byte 1 alone (2^63)", b"\x10" + b"\x80" * 9 + b"\x01" + K),
        ("10th byte 2", b"\x18" + b"\xff" * 9 + b"\x02"),
        ("10th byte 0x81", b"\x18" + b"\xff" * 9 + b"\x81"),
        ("10th byte 0x81 then 00", b"\x18" + b"\xff" * 9 + b"\x81\x00"),
        ("eleven bytes", b"\x10" + b"\x80" * 10 + b"\x00"),
        ("10th byte 2 in an unknown field", K + b"\x48" + b"\xff" * 9 + b"\x02"),
        ("10th byte 2 in a tag", b"\xff" * 9 + b"\x02"),
    ]
    full = uv(U64)
    for k in range(1, len(full)):
        out.append(("valueOffset cut after byte %d of 10" % k, b"\x10" + full[:k]))
    out.append(("checksum cut after byte 1 of 2", K + b"\x18\x80"))
    out.append(("length cut after byte 1 of 2", b"\x0a\x80"))
    out.append(("tag cut after byte 1 of 2", K + b"\x8a"))
    return out


def _tags():
    big = uv(((1 << 32) + 1) << 3 | 2)
    out = [
        ("tag 8a 00 for the key", b"\x8a\x00\x01k"),
        ("tag 90 80 00 for valueOffset", b"\x90\x80\x00\x07" + K),
        ("field 0 varint", b"\x00\x00"),
        ("field 0 bytes", b"\x02\x01k"),
        ("field 0 after a key", K + b"\x00\x00"),
        ("field 2^29-1 varint", field(MAX_FIELD, 5, 0) + K),
        ("field 2^29-1 bytes", K + field(MAX_FIELD, b"xy") + VO),
        ("field 2^29 varint", field(MAX_FIELD + 1, 5, 0) + K),
        ("field 2^29 bytes", K + field(MAX_FIELD + 1, b"xy")),
        ("field 2^32+1 bytes", big + b"\x01k"),
        ("field 2^32+1 bytes after a key", field(1, b"first") + big + b"\x01k"),
        ("field 2^32+2 varint", uv(((1 << 32) + 2) << 3) + b"\x07"),
        ("field 2^61-1 bytes", uv(U64 & ~7 | 2) + b"\x01k"),
    ]
    for wt in (4, 6, 7):
        out.append(("field 5 wire type %d" % wt, tag(5, wt)))
        out.append(("field 1 wire type %d" % wt, tag(1, wt) + b"\x01k"))
        out.append(("field 2 wire type %d after a key" % wt, K + tag(2, wt) + b"\x07"))
    return out


def _lengths():
    return [
        ("key of length 0", b"\x0a\x00"),
        ("key of length 0 then valueOffset", b"\x0a\x00" + VO),
        ("key fills the record", b"\x0a\x03abc"),
        ("key one byte too long", b"\x0a\x04abc"),
        ("key one byte too long after fields", VO + CS + b"\x0a\x02a"),
        ("key of 2^32+3 with 3 bytes there", b"\x0a" + uv((1 << 32) + 3) + b"abc"),
        ("key of 2^32 with nothing there", b"\x0a" + uv(1 << 32)),
        ("key of 2^64-1", b"\x0a" + uv(U64) + b"abc"),
        ("key of 2^64-1 after a field", VO + b"\x0a" + uv(U64) + b"abc"),
        ("key of 2^63", b"\x0a" + uv(1 << 63) + b"abc"),
        ("unknown bytes of 2^32+2 with 2 there", K + b"\x4a" + uv((1 << 32) + 2) + b"xy"),
        ("unknown bytes of 2^64-1", K + b"\x4a" + uv(U64) + b"xy"),
        ("unknown bytes fill the record", K + b"\x4a\x02xy"),
        ("unknown bytes one too long", K + b"\x4a\x03xy"),
        ("ends after the key's tag", b"\x0a"),
        ("ends after valueOffset's tag", K + b"\x10"),
        ("ends after an unknown tag", K + b"\x4a"),
        ("ends after the key's length", b"\x0a\x03"),
        ("ends after an unknown length", K + b"\x4a\x01"),
    ]


def _fixed():
    return [
        ("fixed32 with 3 bytes left", K + tag(9, 5) + b"\x01\x02\x03"),
        ("fixed32 with 4 bytes left", K + tag(9, 5) + b"\x01\x02\x03\x04"),
        ("fixed32 with nothing left", K + tag(9, 5)),
        ("fixed64 with 7 bytes left", K + tag(9, 1) + b"\x01\x02\x03\x04\x05\x06\x07"),
        ("fixed64 with 8 bytes left", K + tag(9, 1) + b"\x01\x02\x03\x04\x05\x06\x07\x08"),
        ("fixed64 whose second half reads as fields", tag(9, 1) + F64),
        ("fixed64 whose second half reads as fields, then a key", tag(9, 1) + F64 + K),
        ("fixed32 that reads as fields", tag(9, 5) + F32 + K),
        ("fixed64 then fixed32 then fields", tag(9, 1) + F64 + tag(9, 5) + F32 + field(2, 8, 0)),
    ]


def _wrong_types():
    out = []
    forms = [
        ("key as varint", field(1, 5, 0), field(1, b"good")),
        ("key as fixed32", tag(1, 5) + F32, field(1, b"good")),
        ("key as fixed64", tag(1, 1) + F64, field(1, b"good")),
        ("valueOffset as bytes", field(2, b"xy"), field(2, 77, 0)),
        ("valueOffset as fixed64", tag(2, 1) + b"\x01" * 8, field(2, 77, 0)),
        ("valueOffset as fixed32", tag(2, 5) + b"\x01" * 4, field(2, 77, 0)),
        ("checksum as bytes", field(3, b"\x10\x05"), field(3, 88, 0)),
        ("checksum as fixed64", tag(3, 1) + b"\x02" * 8, field(3, 88, 0)),
    ]
    for name, wrong, good in forms:
        out.append((name + " alone", wrong))
        out.append((name + " before a good one", wrong + good))
        out.append((name + " after a good one", good + wrong))
    return out


def _repeats():
    return [
        ("fields in order 3, 2, 1", CS + VO + K),
        ("key twice", field(1, b"a") + field(1, b"b")),
        ("key twice, the second empty", field(1, b"a") + field(1, b"")),
        ("key twice, the first empty", field(1, b"") + field(1, b"bc") + VO),
        ("valueOffset three times", field(2, 1, 0) + field(2, 1 << 40, 0) + field(2, 3, 0)),
        ("checksum twice, the second 0", field(3, 9, 0) + field(3, 0, 0)),
        ("key, fields, key", field(1, b"a") + VO + CS + field(1, b"zz")),
        ("the empty record", b""),
    ]


def _groups():
    every = (field(1, b"in") + field(2, 3, 0) + field(9, b"\x01\x02\x03\x04", 5) + field(9, b"\x01" * 8, 1) +
             field(3, 4, 0) + group(6))
    return [
        ("empty group", group(5) + K),
        ("group after the fields", K + VO + group(5)),
        ("group holding every wire type", group(5, every) + K + VO),
        ("group inside a group", group(5, group(6, field(1, b"x"))) + K),
        ("group with a five-byte tag", group(MAX_FIELD, field(2, 1, 0)) + VO),
        ("16 nested groups", nested_groups(16) + K),
        ("17 nested groups", nested_groups(17) + K),
        ("16 nested groups inside nothing, twice", nested_groups(16) + nested_groups(16, 9)),
        ("end tag of another number", tag(5, 3) + tag(6, 4)),
        ("inner end tag of another number", tag(5, 3) + tag(6, 3) + tag(5, 4) + tag(6, 4)),
        ("end tag with no start", tag(5, 4)),
        ("end tag with no start after a group", group(5) + tag(5, 4)),
        ("start with no end", tag(5, 3)),
        ("start with no end around a key", tag(5, 3) + K),
        ("bytes in a group run past the record", tag(5, 3) + b"\x0a\x05ab" + tag(5, 4)),
        ("fixed64 in a group runs past the record", tag(5, 3) + tag(9, 1) + b"\x01" * 6 + tag(5, 4)),
        ("fixed64 in a group whose second half reads as an end tag", tag(5, 3) + tag(9, 1) + b"\x01" * 4 + tag(5, 4) +
         b"\x01" * 3 + tag(5, 4) + K),
        ("group whose field number is 1", group(1, field(1, b"in")) + K),
        ("group 1 alone", group(1)),
        ("group 2 holding a valueOffset", VO + group(2, field(2, 99, 0))),
        ("group 3 before a checksum", group(3, field(3, 99, 0)) + CS),
        ("field 0 in a group", tag(5, 3) + b"\x00\x00" + tag(5, 4)),
        ("field 2^29 in a group", tag(5, 3) + field(MAX_FIELD + 1, 1, 0) + tag(5, 4)),
        ("wire type 6 in a group", tag(5, 3) + tag(7, 6) + tag(5, 4)),
        ("wire type 7 in a group", tag(5, 3) + tag(7, 7) + tag(5, 4)),
        ("10th byte 2 in a group", tag(5, 3) + b"\x48" + b"\xff" * 9 + b"\x02" + tag(5, 4)),
        ("length 2^32+1 in a group", tag(5, 3) + b"\x4a" + uv((1 << 32) + 1) + b"x" + tag(5, 4)),
    ]


def index_families():
    """family name -> [(case name, IndexEntry record)]"""
    return {"varints": _varints(), "tags": _tags(), "lengths": _lengths(), "fixed": _fixed(),
            "wrong wire type": _wrong_types(), "repeats and order": _repeats(), "groups": _groups()}


def data_family():
    """[(case name, DataEntry record)]: the skip, fixed, group and length forms around field 1."""
    v = field(1, b"val")
    out = [
        ("absent", b""),
        ("present and empty", b"\x0a\x00"),
        ("only an unknown field", field(2, 7, 0)),
        ("present", v),
        ("last occurrence wins", field(1, b"old") + v),
        ("last occurrence wins, empty", v + field(1, b"")),
        ("field 1 as a varint", field(1, 5, 0)),
        ("field 1 as a varint, then the value", field(1, 5, 0) + v),
        ("the value, then field 1 as a varint", v + field(1, 5, 0)),
        ("field 1 as fixed64 that reads as a value", tag(1, 1) + b"\x6b\x6c\x6d\x6e\x0a\x02zz"),
        ("field 1 as fixed32 that reads as a value", tag(1, 5) + b"\x0a\x02zz" + v),
        ("unknown fields around it", field(2, b"abc") + v + field(3, 7, 0)),
        ("tag 8a 00", b"\x8a\x00\x03val"),
        ("length in three bytes", b"\x0a" + uv(3, 3) + b"val"),
        ("value fills the record", b"\x0a\x03abc"),
        ("value one byte too long", b"\x0a\x04abc"),
        ("value of 2^32+3 with 3 bytes there", b"\x0a" + uv((1 << 32) + 3) + b"abc"),
        ("value of 2^64-1", b"\x0a" + uv(U64) + b"abc"),
        ("ends after the tag", b"\x0a"),
        ("ends after the length", v + b"\x0a\x02"),
        ("unknown bytes of 2^32+2", v + b"\x4a" + uv((1 << 32) + 2) + b"xy"),
        ("field 0", b"\x00\x00"),
        ("field 2^29-1", field(MAX_FIELD, 5, 0) + v),
        ("field 2^29", field(MAX_FIELD + 1, 5, 0) + v),
        ("field 2^32+1 bytes", uv(((1 << 32) + 1) << 3 | 2) + b"\x03val"),
        ("wire type 4", v + tag(5, 4)),
        ("wire type 6", tag(1, 6) + v),
        ("wire type 7", v + tag(2, 7)),
        ("10th byte 1", b"\x10" + b"\xff" * 9 + b"\x01" + v),
        ("10th byte 2", b"\x10" + b"\xff" * 9 + b"\x02" + v),
        ("varint cut", v + b"\x10\x80"),
        ("fixed32 with 3 bytes left", v + tag(9, 5) + b"\x01\x02\x03"),
        ("fixed32 with 4 bytes left", v + tag(9, 5) + b"\x01\x02\x03\x04"),
        ("fixed64 with 7 bytes left", v + tag(9, 1) + b"\x01" * 7),
        ("fixed64 with 8 bytes left", v + tag(9, 1) + b"\x01" * 8),
        ("fixed64 whose second half reads as a value", tag(9, 1) + b"\x6b\x6c\x6d\x6e\x0a\x02zz"),
        ("empty group", group(5) + v),
        ("group holding a value", v + group(5, field(1, b"inner"))),
        ("group whose field number is 1", group(1, field(1, b"inner")) + v),
        ("group 1 alone", group(1, field(1, b"inner"))),
        ("16 nested groups", nested_groups(16) + v),
        ("17 nested groups", nested_groups(17) + v),
        ("end tag of another number", v + tag(5, 3) + tag(6, 4)),
        ("start with no end", tag(5, 3) + v),
        ("bytes in a group run past the record", tag(5, 3) + b"\x0a\x05ab" + tag(5, 4)),
    ]
    return out


def all_index_cases():
    return [(fam + ": " + name, rec) for fam, cases in index_families().items() for name, rec in cases]


# ---- seeded records --------------------------------------------------------------------------------------
def _piece(rng, depth=0):
    """One field, mostly well formed."""
    if rng.random() < 0.18:  # malformed on purpose
        return rng.choice((
            b"\x00\x01", tag(5, 4), tag(rng.choice((1, 2, 7)), rng.choice((6, 7))), field(MAX_FIELD + 1, 1, 0),
            b"\x0a" + uv(rng.choice((1 << 32, U64, 200))) + b"k",
            b"\x10" + b"\xff" * 9 + bytes([rng.choice((2, 0x7F, 0x81))]),
            uv(((1 << 32) + 1) << 3 | 2) + b"\x01k", tag(5, 3) + tag(6, 4), tag(9, 3)))
    r = rng.random()
    if r < 0.22:
        return field(1, rng.randbytes(rng.choice((0, 1, 3, 8, 21))))
    if r < 0.36:
        return field(rng.choice((2, 3)), rng.choice(EDGE_VALUES + (rng.getrandbits(rng.randint(1, 64)),)), 0)
    if r < 0.44:
        return tag(rng.choice((2, 3)), 0) + uv(rng.getrandbits(20), rng.randint(1, 10))
    if r < 0.52:
        return field(rng.choice((4, 15, 16, 2047, MAX_FIELD)), rng.randbytes(rng.randint(0, 19)))
    if r < 0.58:
        return field(rng.choice((1, 4, 300)), rng.getrandbits(rng.randint(1, 64)), 0)
    if r < 0.64:
        return field(rng.choice((1, 2, 3, 9)), rng.randbytes(4), 5)
    if r < 0.70:
        return field(rng.choice((1, 2, 3, 9)), rng.randbytes(8), 1)
    if r < 0.76:
        return field(rng.choice((2, 3)), rng.randbytes(rng.randint(0, 5)))
    if r < 0.88 and depth < 3:
        return group(rng.choice((1, 2, 5, 1000)), b"".join(_piece(rng, depth + 1) for _ in range(rng.randint(0, 3))))
    if r < 0.94:
        return nested_groups(rng.choice((2, 15, 16, 17)))
    return uv(rng.choice((1, 2, 9)) << 3 | 2, rng.randint(2, 5)) + b"\x02hi"


def seeded_records(seed, n):
    """n records assembled from such pieces; about a third of them are cut at a random byte."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        rec = b"".join(_piece(rng) for _ in range(rng.randint(0, 4)))
        if rec and rng.random() < 1 / 3:
            rec = rec[:rng.randrange(len(rec))]
        out.append(rec)
    return out


# ---- well-formed but non-canonical encodings of a given entry -----------------------------------------------
JUNK20 = field(15, bytes(range(0x61, 0x75)))       # an unknown bytes field of 22 bytes
JUNK40 = field(2047, bytes(range(0x30, 0x58)))     # one of 43 bytes
GROUPS = group(5, field(1, b"not the key") + group(6, field(2, 1, 0)) + field(9, b"\x01" * 8, 1))


def _dec_reversed(k, vo, cs):
    return field(3, cs, 0) + field(2, vo, 0) + field(1, k)


def _dec_padded(k, vo, cs):
    return b"\x8a\x00" + uv(len(k), 3) + k + b"\x90\x80\x00" + uv(vo, 10) + b"\x98\x00" + uv(cs, 10)


def _dec_unknown_between(k, vo, cs):
    return (field(MAX_FIELD, 5, 0) + field(1, k) + JUNK20 + field(2, vo, 0) + field(9, b"\x01\x02\x03\x04", 5) +
            field(3, cs, 0) + tag(9, 1) + F64[:4] + b"\x01\x02\x03\x04")


def _dec_groups_between(k, vo, cs):
    return GROUPS + field(1, k) + nested_groups(16) + field(2, vo, 0) + group(1, K) + field(3, cs, 0) + GROUPS


def _dec_repeated(k, vo, cs):
    return (field(1, b"an earlier key, longer than the last") + field(2, vo ^ 1, 0) + field(3, cs ^ U64, 0) +
            field(2, 1 << 63, 0) + field(1, k) + field(2, vo, 0) + field(3, cs, 0))


def _dec_wrong_types_after(k, vo, cs):
    return (field(1, k) + field(2, vo, 0) + field(3, cs, 0) + field(1, 5, 0) + tag(1, 1) + F64 + field(2, b"xy") +
            tag(3, 5) + F32)


def _dec_far_key(k, vo, cs):
    return field(2, vo, 0) + field(3, cs, 0) + JUNK40 + b"\x0a" + uv(len(k), 2) + k + JUNK40


DECORATIONS = (_dec_reversed, _dec_padded, _dec_unknown_between, _dec_groups_between, _dec_repeated,
               _dec_wrong_types_after, _dec_far_key)


def decorated(key, vo, cs, j):
    """A well-formed, non-canonical IndexEntry record of (key, vo, cs); j picks the form."""
    return DECORATIONS[j % len(DECORATIONS)](key, vo, cs)
