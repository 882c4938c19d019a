"""WAL recovery, the parts that need no GPU: simpledb.proto's host mirror of proto.Unmarshal(WalMutation) against
hand-written vectors (one or more per parse rule) and, where google.protobuf is importable, against a message
class built at run time from the field numbers; the marshal helpers; the model the GPU tests compare with; and
the argument errors of rio_wal_ops_plan / rio_wal_ops_gather, which return before any device call."""
import ctypes
import random

import pytest

import wal_model as WM
from recordio import _lib as L
from simpledb import proto as P
from wal_model import field, group, nested_groups

A, D = P.ADDITION, P.DELETE_TOMBSTONE


def um(b):
    m = P.unmarshal_wal_mutation(b)
    return m.member, m.key, m.value, m.keyBytes, m.valueBytes


# ---- marshal ---------------------------------------------------------------------------------------------

def test_marshal_matches_fixed_bytes():
    assert P.marshal_upsert(b"k", b"vv") == bytes.fromhex("0a07" "1a016b" "22027676")
    assert P.marshal_delete(b"key") == bytes.fromhex("1205" "12036b6579")
    assert P.marshal_upsert_str("k", "é") == bytes.fromhex("0a07" "0a016b" "1202c3a9")
    assert P.marshal_delete_str("k") == bytes.fromhex("1203" "0a016b")
    # proto3 defaults are omitted, the oneof member itself is not
    assert P.marshal_upsert(b"", b"") == b"\x0a\x00" and P.marshal_delete(b"") == b"\x12\x00"
    assert P.marshal_upsert(b"k", b"") == bytes.fromhex("0a03" "1a016b")
    big = P.marshal_upsert(b"k" * 200, b"v" * 70000)
    body = (1 + 2 + 200) + (1 + 3 + 70000)  # tag, length varint, payload of each field
    assert big[:4] == b"\x0a" + P.put_varint(body) and len(big) == 4 + body
    assert big[4:7] == b"\x1a\xc8\x01" and big[207:211] == b"\x22\xf0\xa2\x04"


def test_marshal_round_trips():
    rng = random.Random(1)
    for _ in range(200):
        k, v = rng.randbytes(rng.randint(0, 300)), rng.randbytes(rng.randint(0, 300))
        assert um(P.marshal_upsert(k, v)) == (A, b"", b"", k, v)
        assert um(P.marshal_delete(k)) == (D, b"", b"", k, b"")
    assert um(P.marshal_upsert_str("schlüssel", "wert €")) == (A, "schlüssel".encode(), "wert €".encode(), b"", b"")
    assert um(P.marshal_delete_str("\U0001F600")) == (D, "\U0001F600".encode(), b"", b"", b"")


# ---- the parse rules, one by one -------------------------------------------------------------------------

def test_no_member_is_no_op():
    for rec in (None, b"", field(3, b"unknown"), field(1, 5, 0), field(2, b"12345678", 1), field(1, b"1234", 5)):
        assert um(rec)[0] is None and WM.classify(rec) == (0, None), rec


def test_members_and_their_fields():
    assert um(field(1, field(1, b"k") + field(2, b"v") + field(3, b"kb") + field(4, b"vb"))) == (A, b"k", b"v", b"kb", b"vb")
    assert um(field(2, field(1, b"k") + field(2, b"kb"))) == (D, b"k", b"", b"kb", b"")
    # deleteTombStone has no fields 3 and 4: skipped as unknown
    assert um(field(2, field(3, b"x") + field(4, b"y"))) == (D, b"", b"", b"", b"")


def test_last_member_wins_and_a_switch_starts_empty():
    add, dele = field(1, field(3, b"ka") + field(4, b"va")), field(2, field(2, b"kd"))
    assert um(add + dele) == (D, b"", b"", b"kd", b"")
    assert um(dele + add) == (A, b"", b"", b"ka", b"va")
    # back to the first member: it starts empty again, the earlier occurrence is gone
    assert um(add + dele + field(1, field(4, b"only v"))) == (A, b"", b"", b"", b"only v")


def test_repeated_member_merges_field_by_field():
    rec = field(1, field(3, b"k1") + field(4, b"v1")) + field(1, field(4, b"v2") + field(1, b"s"))
    assert um(rec) == (A, b"s", b"", b"k1", b"v2")
    rec = field(2, field(1, b"a")) + field(2, field(2, b"b")) + field(2, b"")
    assert um(rec) == (D, b"a", b"", b"b", b"")
    # inside one occurrence the last occurrence of a field wins
    assert um(field(1, field(3, b"x") + field(3, b"yy")))[3] == b"yy"


def test_other_wire_types_and_unknown_fields_are_skipped_at_both_levels():
    inner = field(3, 7, 0) + field(4, b"12345678", 1) + field(1, b"1234", 5) + field(9, b"u") + field(3, b"kb") + field(4, b"vb")
    rec = field(1, 1, 0) + field(2, b"4444", 5) + field(1, b"88888888", 1) + field(77, b"unknown") + field(1, inner)
    assert um(rec) == (A, b"", b"", b"kb", b"vb")
    # a member with wire type 0 does not switch the oneof
    assert um(field(2, field(2, b"kd")) + field(1, 1, 0))[0] == D


def test_groups():
    ok = field(1, field(3, b"k") + field(4, b"v"))
    assert um(group(5, field(1, b"x") + group(6)) + ok)[0] == A
    assert um(field(1, group(5, field(1, b"\xff")) + field(3, b"k") + field(4, b"v"))) == (A, b"", b"", b"k", b"v")
    assert um(nested_groups(16) + ok)[0] == A
    for bad in (nested_groups(17) + ok, P.put_varint(5 << 3 | 3) + P.put_varint(6 << 3 | 4), P.put_varint(5 << 3 | 4),
                P.put_varint(5 << 3 | 3), field(1, P.put_varint(5 << 3 | 3)) + P.put_varint(5 << 3 | 4)):
        with pytest.raises(P.WireError):
            um(bad)


def test_malformed_wire_data_at_either_level():
    ok = field(1, field(3, b"k") + field(4, b"v"))
    ten = lambda last: b"\x80" * 9 + bytes([last])  # noqa: E731
    assert um(field(9, 1 << 63, 0) + ok)[0] == A and field(9, 1 << 63, 0)[1:] == ten(1)
    bad = [b"\x08" + ten(2) + ok,                       # a varint whose 10th byte is 2
           b"\x08" + b"\x80" * 10 + b"\x00",           # an 11-byte varint
           b"\x00\x00",                                  # field number 0
           P.put_varint(0x20000000 << 3 | 0) + b"\x00",  # field number past 2^29 - 1
           b"\x0e", b"\x0f\x00",                        # wire types 6 and 7
           b"\x0a\x05\x1a\x01k",                        # the member's length leaves the record
           b"\x0a\x03\x1a\x05k",                        # a field's length leaves the member
           b"\x0a\x04\x1a\x01k\x22",                   # a tag at the member's end without its length
           b"\x0a", b"\x0a\x80", b"\x09\x01\x02",     # cut inside a length / a fixed64
           field(1, b"\x18\x80"), field(1, b"\x1d\x00"), field(2, b"\x00")]
    for rec in bad:
        with pytest.raises(P.WireError):
            um(rec)
        assert WM.classify(rec) == (WM.PROTO, None)
    assert um(b"\x08" + ten(1) + ok)[0] == A


UTF8_BAD = [b"\xc0\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\x80", b"\xe2\x82", b"\xc1\xbf", b"\xf5\x80\x80\x80",
            b"\xe0\x9f\xbf", b"\xf0\x8f\xbf\xbf", b"ab\xff", b"\xc3", b"\xc3\x28"]
UTF8_OK = [b"", b"ascii", "é€\U0001F600".encode(), b"\xed\x9f\xbf", b"\xee\x80\x80", b"\xf4\x8f\xbf\xbf", b"\xe0\xa0\x80",
           b"\xf0\x90\x80\x80", b"\x00"]


def test_string_fields_must_be_utf8_bytes_fields_need_not():
    for s in UTF8_OK:
        assert P.utf8_valid(s) and um(field(1, field(1, s) + field(2, s))) == (A, s, s, b"", b"")
    for s in UTF8_BAD:
        assert not P.utf8_valid(s)
        for rec in (field(1, field(1, s)), field(1, field(2, s)), field(2, field(1, s)),
                    field(1, field(1, s) + field(1, b"replaced")), field(1, field(1, b"ok") + field(2, s) + field(2, b"ok"))):
            with pytest.raises(P.InvalidUTF8Error):
                um(rec)
            assert WM.classify(rec) == (WM.UTF8, None)
        assert um(field(1, field(3, s) + field(4, s))) == (A, b"", b"", s, s)
        assert um(field(2, field(2, s))) == (D, b"", b"", s, b"")
        # a string field with another wire type is skipped, not checked
        assert um(field(1, field(1, b"\xff\xff\xff\xff", 5)))[0] == A
    with pytest.raises(P.InvalidUTF8Error) as e:
        um(field(1, field(2, b"\xff")))
    assert e.value.field == "proto.UpsertMutation.value"
    # the first error in wire order is the record's
    assert WM.classify(field(1, field(1, b"\xff")) + b"\x0f") == (WM.UTF8, None)
    assert WM.classify(b"\x0a\x05\x0a\x01\xff") == (WM.PROTO, None)  # the member's length fails before its field is read


def test_the_switch():
    c = WM.classify
    assert c(P.marshal_upsert(b"k", b"v")) == (0, (b"k", b"v"))
    assert c(P.marshal_delete(b"k")) == (0, (b"k", None))
    assert c(P.marshal_upsert_str("k", "")) == (0, (b"k", b""))  # an empty string value is non-nil
    assert c(P.marshal_upsert(b"", b"")) == (0, (b"", b""))      # no keyBytes: the string pair, both empty
    assert c(field(1, field(3, b"kb") + field(1, b"s") + field(2, b"sv") + field(4, b"vb"))) == (0, (b"kb", b"vb"))
    assert c(field(1, field(4, b"vb") + field(1, b"s"))) == (0, (b"s", b""))  # valueBytes alone is not read
    assert c(field(1, field(3, b"kb"))) == (WM.VALUE_NIL, None)
    assert c(field(1, field(3, b"kb") + field(4, b""))) == (WM.VALUE_NIL, None)
    assert c(field(1, field(3, b"kb") + field(4, b"v") + field(4, b""))) == (WM.VALUE_NIL, None)
    assert c(field(2, field(1, b"s") + field(2, b"kb"))) == (0, (b"kb", None))
    assert c(field(2, field(1, b"s") + field(2, b""))) == (0, (b"s", None))
    assert c(P.marshal_delete(b"")) == (0, (b"", None))


def test_model_arrays():
    recs = [P.marshal_upsert(b"b", b"1"), b"", None, P.marshal_delete(b"b"), field(9, b"x"), P.marshal_upsert_str("a", ""),
            P.marshal_upsert(b"ccc", b"22")]
    e = WM.expected(recs)
    assert e["result"] == [7, 4, 6, 3, 3, WM.NONE, 0, 0]
    assert e["ops"] == [(b"b", b"1"), (b"b", None), (b"a", b""), (b"ccc", b"22")] and e["op_rec"] == [0, 3, 5, 6]
    assert (e["keys"], e["values"]) == (b"bbaccc", b"122") and e["flags"] == [0, 1, 0, 0]
    assert e["key_off"] == [0, 1, 2, 3, 6] and e["val_off"] == [0, 1, 1, 1, 3]
    e = WM.expected(recs + [b"\x0f", field(1, field(1, b"\xff"))])
    assert e["result"][5:7] == [7, WM.PROTO]
    assert WM.expected([])["result"] == [0, 0, 0, 0, 0, WM.NONE, 0, 0]


# ---- against google.protobuf -----------------------------------------------------------------------------

def _message_class():
    pb = pytest.importorskip("google.protobuf")
    del pb
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

    F = descriptor_pb2.FieldDescriptorProto
    fdp = descriptor_pb2.FileDescriptorProto(name="wal_mutation_mirror.proto", package="proto", syntax="proto3")
    up = fdp.message_type.add(name="UpsertMutation")
    for num, name, typ in ((1, "key", F.TYPE_STRING), (2, "value", F.TYPE_STRING), (3, "keyBytes", F.TYPE_BYTES),
                           (4, "valueBytes", F.TYPE_BYTES)):
        up.field.add(name=name, number=num, type=typ, label=F.LABEL_OPTIONAL)
    de = fdp.message_type.add(name="DeleteTombstoneMutation")
    for num, name, typ in ((1, "key", F.TYPE_STRING), (2, "keyBytes", F.TYPE_BYTES)):
        de.field.add(name=name, number=num, type=typ, label=F.LABEL_OPTIONAL)
    wm = fdp.message_type.add(name="WalMutation")
    wm.oneof_decl.add(name="mutation")
    wm.field.add(name="addition", number=1, type=F.TYPE_MESSAGE, type_name=".proto.UpsertMutation",
                 label=F.LABEL_OPTIONAL, oneof_index=0)
    wm.field.add(name="deleteTombStone", number=2, type=F.TYPE_MESSAGE, type_name=".proto.DeleteTombstoneMutation",
                 label=F.LABEL_OPTIONAL, oneof_index=0)
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fdp)
    return message_factory.GetMessageClass(pool.FindMessageTypeByName("proto.WalMutation"))


def _by_protobuf(cls, rec):
    from google.protobuf.message import DecodeError

    msg = cls()
    try:
        msg.ParseFromString(rec or b"")
    except DecodeError:
        return None
    which = msg.WhichOneof("mutation")
    if which == "addition":
        a = msg.addition
        return A, a.key.encode(), a.value.encode(), a.keyBytes, a.valueBytes
    if which == "deleteTombStone":
        d = msg.deleteTombStone
        return D, d.key.encode(), b"", d.keyBytes, b""
    return None, b"", b"", b"", b""


def _by_mirror(rec):
    try:
        return um(rec)
    except ValueError:
        return None


@pytest.mark.parametrize("family", ["ordinary", "merges", "malformed"])
def test_mirror_agrees_with_protobuf_on_the_seeded_corpus(family):
    cls = _message_class()
    recs = WM.corpus(2024)[family]
    assert len(recs) == 300
    got = [_by_mirror(r) for r in recs]
    want = [_by_protobuf(cls, r) for r in recs]
    diff = [(r.hex() if r else r, g, w) for r, g, w in zip(recs, got, want) if g != w]
    assert not diff, diff[:5]
    if family == "malformed":
        assert 30 < sum(g is None for g in got) < 270  # both outcomes are exercised
    else:
        assert all(g is not None for g in got)


def test_protobuf_agrees_on_the_hand_vectors():
    cls = _message_class()
    add, dele = field(1, field(3, b"ka") + field(4, b"va")), field(2, field(2, b"kd"))
    vectors = [add + dele, dele + add, add + dele + field(1, field(4, b"only v")),
               field(1, field(3, b"k1") + field(4, b"v1")) + field(1, field(4, b"v2") + field(1, b"s")),
               field(2, field(1, b"a")) + field(2, field(2, b"b")) + field(2, b""),
               field(2, field(2, b"kd")) + field(1, 1, 0), group(5, field(1, b"x") + group(6)) + add,
               field(1, group(5, field(1, b"\xff")) + field(3, b"k")), b"\x0a\x05\x1a\x01k", b"\x0a\x03\x1a\x05k", b"\x0e",
               P.put_varint(5 << 3 | 3) + P.put_varint(6 << 3 | 4), P.put_varint(5 << 3 | 4)]
    vectors += [field(1, field(1, s)) for s in UTF8_BAD + UTF8_OK] + [field(1, field(3, s)) for s in UTF8_BAD]
    vectors += [field(1, field(1, UTF8_BAD[0]) + field(1, b"replaced"))]
    for rec in vectors:
        assert _by_mirror(rec) == _by_protobuf(cls, rec), rec.hex()


# ---- rio_wal_ops_plan / rio_wal_ops_gather: argument errors ------------------------------------------------

def test_wal_ops_argument_errors_return_before_any_device_call():
    lib = L.lib()
    # As in test_memstore_host.py: no context can be created without a device, so ctx is a placeholder that is
    # never read: both entry points check their arguments before the first read of *ctx.
    page = ctypes.create_string_buffer(1 << 16)
    ctx = ctypes.addressof(page)
    buf = ctypes.addressof(ctypes.create_string_buffer(64))
    segs = (L.WalSegment * 2)()
    s = ctypes.addressof(segs)
    plan, gather = lib.rio_wal_ops_plan, lib.rio_wal_ops_gather
    assert plan(None, s, 1, buf, None) == L.RIO_ERR_ARG
    assert plan(ctx, None, 1, buf, None) == L.RIO_ERR_ARG
    assert plan(ctx, s, 1, None, None) == L.RIO_ERR_ARG
    assert plan(ctx, s, 0, buf, None) == L.RIO_ERR_ARG
    fields = ("out", "out_off", "flags")
    segs[1].n = 1  # records without arrays
    for missing in fields:
        for f in fields:
            setattr(segs[1], f, None if f == missing else buf)
        assert plan(ctx, s, 2, buf, None) == L.RIO_ERR_ARG, missing
    for f in fields:
        setattr(segs[1], f, buf)
    assert plan(ctx, s, L.RIO_WAL_MAX_SEGMENTS + 1, buf, None) == L.RIO_ERR_UNSUPPORTED
    segs[1].n = (1 << 31) - 1
    assert plan(ctx, s, 2, buf, None) == L.RIO_ERR_UNSUPPORTED
    segs[0].n, segs[1].n = 1 << 30, (1 << 30) - 1  # together 2^31 - 1
    for f in fields:
        setattr(segs[0], f, buf)
    assert plan(ctx, s, 2, buf, None) == L.RIO_ERR_UNSUPPORTED
    assert gather(None, 0, buf, 0, buf, buf, 0, buf, buf, None, None) == L.RIO_ERR_ARG
    assert gather(ctx, 0, buf, 0, None, buf, 0, buf, buf, None, None) == L.RIO_ERR_ARG
    assert gather(ctx, 0, buf, 0, buf, buf, 0, None, buf, None, None) == L.RIO_ERR_ARG
    for k in (2, 5, 8):  # d_keys, d_values, d_flags with ops to write
        args = [ctx, 1, buf, 64, buf, buf, 64, buf, buf, None, None]
        args[k] = None
        assert gather(*args) == L.RIO_ERR_ARG, k
    # a zeroed context has no plan
    assert gather(ctx, 0, buf, 0, buf, buf, 0, buf, buf, None, None) == L.RIO_ERR_STATE
