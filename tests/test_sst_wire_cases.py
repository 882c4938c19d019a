"""The SSTable wire-format families (tests/sst_wire_cases.py) on the CPU: the plain model, the C oracle
(oracle/rio_oracle.c) and the host mirror (sstables/proto.py) agree on every family case and on 20 000 seeded
records, which keeps tests/test_gpu_sst_wire.py's expectations honest; every family holds what its name promises."""
import pytest

import oracle_py as orc
import sst_wire_cases as W
from sstables import proto

SEEDED = W.seeded_records(20260, 20000)


def mirror(rec):
    try:
        return proto.decode_index_entry(rec)
    except ValueError:
        return None


def oracle_data(rec):
    v = orc.data_entry(rec)
    return W.BAD if isinstance(v, orc.BadProto) else v


def three_way_index(name, rec):
    m = W.index_entry_model(rec)
    assert orc.index_entry(rec) == m, ("oracle", name, rec.hex(), m)
    assert mirror(rec) == m, ("mirror", name, rec.hex(), m)
    return m


def two_way_data(name, rec):
    m = W.data_entry_model(rec)
    assert oracle_data(rec) == m, ("oracle", name, rec.hex(), m)
    return m


@pytest.mark.parametrize("family", list(W.index_families()))
def test_index_family_three_way(family):
    cases = W.index_families()[family]
    assert len({n for n, _ in cases}) == len(cases), "case names repeat"
    got = [three_way_index(n, r) for n, r in cases]
    assert any(g is not None for g in got)
    if family not in ("wrong wire type", "repeats and order"):  # skipped or merged: nothing there to reject
        assert any(g is None for g in got)
    # both parsers read every family's cases: an IndexEntry record is a DataEntry record with other names
    for n, r in cases:
        two_way_data(n, r)


def test_data_family_two_way():
    cases = W.data_family()
    assert len({n for n, _ in cases}) == len(cases)
    got = [two_way_data(n, r) for n, r in cases]
    assert any(g is None for g in got) and any(g == b"" for g in got) and any(g is W.BAD for g in got)
    assert sum(1 for g in got if isinstance(g, bytes) and g) >= 10
    for n, r in cases:
        three_way_index(n, r)


def case(family, name):
    return dict(W.index_families()[family])[name]


def test_families_hold_what_they_promise():
    """The answers a reader of the issue expects, spelled out: they hold for the model, and by the tests above
    for the oracle and the mirror."""
    ie, de = W.index_entry_model, W.data_entry_model
    for v in W.EDGE_VALUES:
        assert ie(case("varints", "valueOffset=%#x" % v)) == (b"", v, 0)
        assert ie(case("varints", "checksum=%#x" % v)) == (b"", 0, v)
    assert ie(case("varints", "valueOffset 80 00")) == (b"", 0, 0)
    assert ie(case("varints", "valueOffset nine 80 then 00")) == (b"", 0, 0)
    assert ie(case("varints", "10th byte 1")) == (b"", 0, W.U64)
    assert ie(case("varints", "10th byte 1 alone (2^63)")) == (b"k", 1 << 63, 0)
    for n in ("10th byte 2", "10th byte 0x81", "eleven bytes"):
        assert ie(case("varints", n)) is None
    assert all(ie(case("varints", "valueOffset cut after byte %d of 10" % k)) is None for k in range(1, 10))
    assert ie(case("tags", "tag 8a 00 for the key")) == (b"k", 0, 0)
    assert ie(case("tags", "field 0 varint")) is None
    assert ie(case("tags", "field 2^29-1 varint")) == (b"k", 0, 0)
    assert ie(case("tags", "field 2^29 varint")) is None
    assert ie(case("tags", "field 2^32+1 bytes")) is None
    assert all(ie(case("tags", "field 5 wire type %d" % wt)) is None for wt in (4, 6, 7))
    assert ie(case("lengths", "key of length 0")) == (b"", 0, 0)
    assert ie(case("lengths", "key fills the record")) == (b"abc", 0, 0)
    for n in ("key one byte too long", "key of 2^32+3 with 3 bytes there", "key of 2^64-1", "ends after the key's tag",
              "ends after the key's length"):
        assert ie(case("lengths", n)) is None
    assert ie(case("fixed", "fixed32 with 3 bytes left")) is None
    assert ie(case("fixed", "fixed32 with 4 bytes left")) == (b"k", 0, 0)
    assert ie(case("fixed", "fixed64 with 7 bytes left")) is None
    assert ie(case("fixed", "fixed64 with 8 bytes left")) == (b"k", 0, 0)
    assert ie(case("fixed", "fixed64 whose second half reads as fields")) == (b"", 0, 0)
    assert ie(case("wrong wire type", "key as fixed64 before a good one")) == (b"good", 0, 0)
    assert ie(case("wrong wire type", "key as varint after a good one")) == (b"good", 0, 0)
    assert ie(case("wrong wire type", "valueOffset as bytes after a good one")) == (b"", 77, 0)
    assert ie(case("wrong wire type", "checksum as fixed64 before a good one")) == (b"", 0, 88)
    assert ie(case("repeats and order", "fields in order 3, 2, 1")) == (b"k", 7, 9)
    assert ie(case("repeats and order", "key twice")) == (b"b", 0, 0)
    assert ie(case("repeats and order", "key twice, the second empty")) == (b"", 0, 0)
    assert ie(case("repeats and order", "valueOffset three times")) == (b"", 3, 0)
    assert ie(case("repeats and order", "the empty record")) == (b"", 0, 0)
    assert ie(case("groups", "empty group")) == (b"k", 0, 0)
    assert ie(case("groups", "group holding every wire type")) == (b"k", 7, 0)
    assert ie(case("groups", "16 nested groups")) == (b"k", 0, 0)
    assert ie(case("groups", "group whose field number is 1")) == (b"k", 0, 0)
    for n in ("17 nested groups", "end tag of another number", "end tag with no start", "start with no end",
              "bytes in a group run past the record"):
        assert ie(case("groups", n)) is None
    d = dict(W.data_family())
    assert de(d["absent"]) is None and de(d["present and empty"]) == b"" and de(d["present"]) == b"val"
    assert de(d["last occurrence wins"]) == b"val" and de(d["last occurrence wins, empty"]) == b""
    assert de(d["field 1 as a varint"]) is None and de(d["field 1 as fixed64 that reads as a value"]) is None
    assert de(d["16 nested groups"]) == b"val" and de(d["17 nested groups"]) is W.BAD
    assert de(d["value of 2^32+3 with 3 bytes there"]) is W.BAD and de(d["field 2^32+1 bytes"]) is W.BAD


def test_seeded_records_three_way_and_balanced():
    assert W.seeded_records(20260, 50) == SEEDED[:50] and W.seeded_records(1, 50) != SEEDED[:50]
    accepted = 0
    for i, r in enumerate(SEEDED):
        accepted += three_way_index("seeded %d" % i, r) is not None
        assert (two_way_data("seeded %d" % i, r) is W.BAD) == (W.index_entry_model(r) is None)
    share = accepted / len(SEEDED)
    assert 0.30 <= share <= 0.70, share
    assert 0.25 < sum(1 for r in SEEDED if len(r) > 16) / len(SEEDED)


def test_decorations_say_what_they_were_given():
    for j in range(len(W.DECORATIONS)):
        for key, vo, cs in ((b"", 0, 0), (b"k", 1, 2), (b"a key of some length, over 32 bytes!", W.U64, 1 << 63)):
            rec = W.decorated(key, vo, cs, j)
            assert three_way_index("decoration %d" % j, rec) == (key, vo, cs)
            assert rec != proto.encode_index_entry(key, vo, cs)
    assert max(len(W.decorated(b"k", 1, 2, j)) for j in range(len(W.DECORATIONS))) > 32
