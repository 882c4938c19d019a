"""Compaction of simpledb.DB, the parts that need no GPU: the candidate selection against the transcription of
tests/db_compact_model.py, CompactionMetadata against hand-written bytes and, where google.protobuf is importable,
against a message class built at run time from the field numbers; the compaction_successful file; repair_compactions
over hand-made directories with placeholder files for the tables; the options."""
import os
import random

import pytest

import db_compact_model as cm
import db_write_model as wm
import simpledb as DB
from recordio.writer import encode_file
from simpledb import proto as P
from sstables import proto as SP


def meta(total, n, nulls):
    return SP.MetaData(version=1, numRecords=n, nullValues=nulls, totalBytes=total)


def select(rows, max_size, ratio):
    """The library's selection over [(totalBytes, numRecords, nullValues)] -> (indexes, sum of numRecords)."""
    paths, total = DB.candidate_tables_for_compaction([(f"/base/t{i}", meta(*r)) for i, r in enumerate(rows)], max_size, ratio)
    return [int(os.path.basename(p)[1:]) for p in paths], total


# ---- selection -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("a, want", [
    ([False, True, False, True, False], [False, True, True, True, False]),
    ([False, False, False], [False, False, False]),
    ([False, True, False], [False, True, False]),
    ([True, False, True, False, False], [True, True, True, False, False]),
    ([True, False, False, True, False, True], [True] * 6),
    ([], []),
])
def test_flood_fill(a, want):
    before = list(a)
    assert cm.flood_fill(a) == want and DB.flood_fill(a) == want
    assert a == before  # the argument is left as it was


def test_flood_fill_equals_the_transcription_on_every_mask_of_8():
    for bits in range(256):
        a = [bool(bits >> i & 1) for i in range(8)]
        assert DB.flood_fill(a) == cm.flood_fill(a)


def test_size_limit_and_flood_fill_select_the_run():
    # tables 1 and 3 are below the limit, table 2 is over it and is filled in; 0 and 4 stay out
    rows = [(500, 10, 0), (99, 10, 0), (500, 7, 0), (0, 10, 0), (100, 10, 0)]
    assert select(rows, 100, 1.0) == ([1, 2, 3], 27)
    assert select(rows, 0, 1.0) == ([], 0)  # totalBytes < 0 never holds
    assert select(rows, 501, 1.0) == ([0, 1, 2, 3, 4], 47)


def test_ratio_boundary_is_float32():
    f02 = wm.f32(0.2)
    assert DB.DefaultCompactionRatio == f02 != 0.2
    # 1 / 5 in float32 is float32(0.2): selected at exactly the ratio; in double arithmetic 0.2 < float32(0.2) would not be
    assert select([(10, 5, 1)], 0, f02) == ([0], 5)
    assert select([(10, 5, 1)], 0, 0.2) == ([0], 5)  # the option's value is a float32
    # the neighbours of the boundary: 3 / 16 below, 13 / 64 above
    assert select([(10, 16, 3)], 0, f02) == ([], 0) and select([(10, 64, 13)], 0, f02) == ([0], 64)
    # uint64 -> float32 rounds on the integer: 2^24 + 1 rounds to 2^24 (ties to even), so the quotient is exactly 1.0
    assert select([(10, 1 << 24, (1 << 24) + 1)], 0, 1.0) == ([0], 1 << 24)
    # 2^53 + 2^29 + 1 is above the float32 tie 2^53 + 2^29 and a double in between would lose the 1
    n = (1 << 53) + (1 << 29) + 1
    assert wm.u64_to_f32(n) == DB._u64_to_f32(n) == float((1 << 53) + (1 << 30))
    rng = random.Random(3)
    for _ in range(300):
        rows = [(rng.randrange(200), rng.choice((0, 1, 5, 10, 1 << 30)), 0) for _ in range(rng.randrange(1, 8))]
        rows = [(tb, n, rng.randrange(n + 1)) for tb, n, _ in rows]
        ratio = rng.choice((0.0, 0.2, f02, 0.5, 1.0))
        names, total = cm.candidates([(i,) + r for i, r in enumerate(rows)], 100, ratio)
        assert select(rows, 100, ratio) == (names, total)


def test_a_table_without_records_has_no_ratio():
    assert select([(10, 0, 0)], 0, 0.0) == ([], 0)  # 0 / 0 is never computed
    assert select([(10, 0, 0)], 11, 0.0) == ([0], 0)


def test_ratio_zero_selects_everything_with_records_and_one_only_all_tombstones():
    rows = [(10, 4, 0), (10, 4, 3), (10, 4, 4)]
    assert select(rows, 0, 0.0) == ([0, 1, 2], 12)
    assert select(rows, 0, 1.0) == ([2], 4)


def test_model_compacts_only_above_the_file_threshold():
    m = cm.ModelCompactDB(1 << 30)
    m.tables = [(1, {b"a": b"1", b"b": b"x"}), (2, {b"a": None, b"c": b""}), (4, {b"b": b"y"})]
    assert m.compact({}, 3, 100, 1.0) is None and len(m.tables) == 3  # 3 <= 3
    assert m.compact({1: 100}, 1, 100, 1.0) == [2, 4]  # table 1 is over the limit: the run starts at 2
    # the tombstone of a is dropped with its table, and table 1's value is visible again
    assert m.tables == [(1, {b"a": b"1", b"b": b"x"}), (2, {b"b": b"y"})] and m.get(b"a") == b"1"
    assert m.compact({}, 1, 100, 1.0) == [1, 2] and m.tables == [(1, {b"a": b"1", b"b": b"y"})]
    assert m.compactions == [(2, [2, 4]), (1, [1, 2])]


# ---- CompactionMetadata ----------------------------------------------------------------------------------------

def field(num, payload, wt=2):
    if wt == 2:
        return P.put_varint(num << 3 | 2) + P.put_varint(len(payload)) + payload
    return P.put_varint(num << 3 | wt) + payload


def test_marshal_matches_fixed_bytes():
    m = P.CompactionMetadata("sstable_compaction12", "sstable_000000000000001", ["sstable_000000000000001", "sstable_000000000000002"])
    want = (b"\x0a\x14sstable_compaction12" + b"\x12\x17sstable_000000000000001" + b"\x1a\x17sstable_000000000000001"
            + b"\x1a\x17sstable_000000000000002")
    assert P.marshal_compaction_metadata(m) == want and P.unmarshal_compaction_metadata(want) == m
    # proto3 leaves empty singular strings out; an empty element of the repeated field is written
    assert P.marshal_compaction_metadata(P.CompactionMetadata()) == b""
    assert P.marshal_compaction_metadata(P.CompactionMetadata("", "r", ["", "x"])) == b"\x12\x01r\x1a\x00\x1a\x01x"
    assert P.unmarshal_compaction_metadata(b"\x12\x01r\x1a\x00\x1a\x01x") == P.CompactionMetadata("", "r", ["", "x"])
    assert P.unmarshal_compaction_metadata(None) == P.unmarshal_compaction_metadata(b"") == P.CompactionMetadata()
    long = "p" * 300  # a two-byte length varint, minimal
    assert P.marshal_compaction_metadata(P.CompactionMetadata(long)) == b"\x0a\xac\x02" + long.encode()


def test_round_trips_non_ascii_paths():
    rng = random.Random(5)
    alphabet = "aé€\U0001F600/_0"
    for _ in range(200):
        s = lambda: "".join(rng.choice(alphabet) for _ in range(rng.randrange(0, 12)))  # noqa: E731
        m = P.CompactionMetadata(s(), s(), [s() for _ in range(rng.randrange(0, 5))])
        assert P.unmarshal_compaction_metadata(P.marshal_compaction_metadata(m)) == m


def test_unmarshal_rules():
    um = P.unmarshal_compaction_metadata
    # the last occurrence of a singular field wins, the repeated field appends, in wire order
    assert um(field(1, b"a") + field(3, b"x") + field(1, b"b") + field(3, b"y")) == P.CompactionMetadata("b", "", ["x", "y"])
    # unknown fields and known fields with another wire type are skipped
    rec = field(4, b"unknown") + field(1, b"\x05", 0) + field(2, b"12345678", 1) + field(3, b"1234", 5) + field(2, b"r")
    assert um(rec) == P.CompactionMetadata("", "r", [])
    for bad in (b"\x0a", b"\x0a\x05ab", b"\x00\x00", b"\x0a\xff\xff\xff\xff\xff\xff\xff\xff\xff\x02", b"\x0c"):
        with pytest.raises(P.WireError):
            um(bad)


def test_invalid_utf8_is_an_error_in_every_string_field():
    for num, name in ((1, "writePath"), (2, "replacementPath"), (3, "sstablePaths")):
        for bad in (b"\xff", b"\xc3", b"\xed\xa0\x80", b"\xc0\xaf"):
            with pytest.raises(P.InvalidUTF8Error) as e:
                P.unmarshal_compaction_metadata(field(1, b"ok") + field(num, b"x" + bad))
            assert str(e.value) == f"field proto.CompactionMetadata.{name} contains invalid UTF-8"
    # a path from os.listdir with undecodable bytes (surrogate escapes) is refused on the way out as well
    with pytest.raises(P.InvalidUTF8Error):
        P.marshal_compaction_metadata(P.CompactionMetadata(b"sstable_\xff".decode("utf-8", "surrogateescape")))


def _message_class():
    pb = pytest.importorskip("google.protobuf")
    del pb
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

    F = descriptor_pb2.FieldDescriptorProto
    fdp = descriptor_pb2.FileDescriptorProto(name="compaction_metadata_mirror.proto", package="proto", syntax="proto3")
    msg = fdp.message_type.add(name="CompactionMetadata")
    msg.field.add(name="writePath", number=1, type=F.TYPE_STRING, label=F.LABEL_OPTIONAL)
    msg.field.add(name="replacementPath", number=2, type=F.TYPE_STRING, label=F.LABEL_OPTIONAL)
    msg.field.add(name="sstablePaths", number=3, type=F.TYPE_STRING, label=F.LABEL_REPEATED)
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fdp)
    return message_factory.GetMessageClass(pool.FindMessageTypeByName("proto.CompactionMetadata"))


def test_equals_google_protobuf():
    cls = _message_class()
    from google.protobuf.message import DecodeError

    rng = random.Random(7)
    alphabet = "aé€\U0001F600/_0"
    s = lambda: "".join(rng.choice(alphabet) for _ in range(rng.randrange(0, 12)))  # noqa: E731
    for _ in range(200):
        m = P.CompactionMetadata(s(), s(), [s() for _ in range(rng.randrange(0, 5))])
        g = cls(writePath=m.writePath, replacementPath=m.replacementPath, sstablePaths=m.sstablePaths)
        assert P.marshal_compaction_metadata(m) == g.SerializeToString(deterministic=True)
    # parsing: mutated records, accepted and refused alike
    base = P.marshal_compaction_metadata(P.CompactionMetadata("wé", "r", ["x", "", "y€"])) + field(9, b"u") + field(1, b"\x07", 0)
    for _ in range(400):
        rec = bytearray(base)
        for _ in range(rng.randrange(0, 3)):
            rec[rng.randrange(len(rec))] = rng.randrange(256)
        rec = bytes(rec[:rng.randrange(len(rec) + 1)]) if rng.random() < 0.3 else bytes(rec)
        g = cls()
        try:
            g.ParseFromString(rec)
            want = P.CompactionMetadata(g.writePath, g.replacementPath, list(g.sstablePaths))
        except DecodeError:
            want = None
        try:
            got = P.unmarshal_compaction_metadata(rec)
        except ValueError:
            got = None
        assert got == want, rec


# ---- the compaction_successful file and repairCompactions ---------------------------------------------------------

TABLE_FILES = ("index.rio", "data.rio", "meta.pb.bin", "bloom.bf.gz")


def make_table(base, name, tag):
    d = base / name
    d.mkdir()
    for f in TABLE_FILES:
        (d / f).write_bytes(f"{tag}:{f}".encode())
    return d


def listing(base):
    return sorted(str(p.relative_to(base)) for p in base.rglob("*"))


def test_metadata_file_is_the_writers_default_recordio_file(tmp_path):
    m = P.CompactionMetadata("sstable_compaction1", "sstable_000000000000001", ["sstable_000000000000001", "sstable_000000000000003"])
    assert DB.save_compaction_metadata(str(tmp_path), m) is None
    path = tmp_path / DB.CompactionFinishedSuccessfulFileName
    assert path.name == "compaction_successful"
    assert path.read_bytes() == encode_file([P.marshal_compaction_metadata(m)], 0)  # version 4, uncompressed, one record
    assert DB.read_compaction_metadata(str(path)) == (m, None)
    got, err = DB.read_compaction_metadata(str(tmp_path / "absent"))
    assert got is None and err is not None


def test_metadata_file_damage_is_an_error(tmp_path):
    m = P.CompactionMetadata("sstable_compaction1", "sstable_000000000000001", ["sstable_000000000000001"])
    img = encode_file([P.marshal_compaction_metadata(m)], 0)
    path = tmp_path / "f"
    for cut in range(8, len(img)):  # a header alone, every truncation of the record
        path.write_bytes(img[:cut])
        got, err = DB.read_compaction_metadata(str(path))
        assert got is None and err is not None, cut
    for at in range(8, 8 + 7):  # magic, nil byte, sizes and header checksum: any flipped bit fails the header
        bad = bytearray(img)
        bad[at] ^= 0x10
        path.write_bytes(bytes(bad))
        got, err = DB.read_compaction_metadata(str(path))
        assert got is None and err is not None, at
    path.write_bytes(encode_file([None], 0))  # a nil record is the empty message
    assert DB.read_compaction_metadata(str(path)) == (P.CompactionMetadata(), None)
    path.write_bytes(encode_file([b"\x0a\x01\xff"], 0))  # invalid UTF-8
    got, err = DB.read_compaction_metadata(str(path))
    assert got is None and "invalid UTF-8" in str(err)


def test_repair_deletes_a_compaction_without_metadata(tmp_path):
    make_table(tmp_path, "sstable_000000000000001", "t1")
    make_table(tmp_path, "sstable_000000000000002", "t2")
    make_table(tmp_path, "sstable_compaction123", "c")
    (tmp_path / "wal").mkdir()
    before = [p for p in listing(tmp_path) if not p.startswith("sstable_compaction")]
    assert DB.repair_compactions(str(tmp_path)) is None
    assert listing(tmp_path) == before


def test_repair_deletes_a_compaction_with_truncated_metadata(tmp_path):
    make_table(tmp_path, "sstable_000000000000001", "t1")
    c = make_table(tmp_path, "sstable_compaction9", "c")
    m = P.CompactionMetadata("sstable_compaction9", "sstable_000000000000001", ["sstable_000000000000001"])
    img = encode_file([P.marshal_compaction_metadata(m)], 0)
    (c / DB.CompactionFinishedSuccessfulFileName).write_bytes(img[:-3])
    assert DB.repair_compactions(str(tmp_path)) is None
    assert sorted(os.listdir(tmp_path)) == ["sstable_000000000000001"]
    assert (tmp_path / "sstable_000000000000001" / "data.rio").read_bytes() == b"t1:data.rio"


def finished_compaction(base, inputs, write="sstable_compaction77"):
    c = make_table(base, write, "c")
    m = P.CompactionMetadata(write, inputs[0], list(inputs))
    assert DB.save_compaction_metadata(str(c), m) is None
    return m


def test_repair_finishes_a_compaction_with_every_input_present(tmp_path):
    for g in (1, 2, 3, 4):
        make_table(tmp_path, wm.TABLE_NAME % g, f"t{g}")
    finished_compaction(tmp_path, [wm.TABLE_NAME % 2, wm.TABLE_NAME % 3])
    assert DB.repair_compactions(str(tmp_path)) is None
    assert sorted(os.listdir(tmp_path)) == [wm.TABLE_NAME % 1, wm.TABLE_NAME % 2, wm.TABLE_NAME % 4]
    new = tmp_path / (wm.TABLE_NAME % 2)
    assert sorted(os.listdir(new)) == sorted(TABLE_FILES + (DB.CompactionFinishedSuccessfulFileName,))
    assert (new / "data.rio").read_bytes() == b"c:data.rio"
    assert (tmp_path / (wm.TABLE_NAME % 1) / "data.rio").read_bytes() == b"t1:data.rio"
    assert (tmp_path / (wm.TABLE_NAME % 4) / "data.rio").read_bytes() == b"t4:data.rio"
    after = listing(tmp_path)
    assert DB.repair_compactions(str(tmp_path)) is None and listing(tmp_path) == after  # nothing left to repair


def test_repair_finishes_a_reflect_interrupted_halfway(tmp_path):
    # reflect had removed the replacement and one more input when it was interrupted: 4 is still there, 5 is no input
    for g in (1, 4, 5):
        make_table(tmp_path, wm.TABLE_NAME % g, f"t{g}")
    finished_compaction(tmp_path, [wm.TABLE_NAME % g for g in (2, 3, 4)])
    assert DB.repair_compactions(str(tmp_path)) is None
    assert sorted(os.listdir(tmp_path)) == [wm.TABLE_NAME % 1, wm.TABLE_NAME % 2, wm.TABLE_NAME % 5]
    assert (tmp_path / (wm.TABLE_NAME % 2) / "index.rio").read_bytes() == b"c:index.rio"


def test_repair_of_a_directory_without_compactions_changes_nothing(tmp_path):
    make_table(tmp_path, wm.TABLE_NAME % 1, "t1")
    before = listing(tmp_path)
    assert DB.repair_compactions(str(tmp_path)) is None and listing(tmp_path) == before
    assert DB.repair_compactions(str(tmp_path / "absent")) is not None


# ---- options ------------------------------------------------------------------------------------------------------

def test_constants_and_options(tmp_path):
    assert DB.CompactionFinishedSuccessfulFileName == "compaction_successful"
    assert DB.NumSSTablesToTriggerCompaction == 10 and DB.DefaultCompactionMaxSizeBytes == 5 << 30
    assert DB.DefaultCompactionRatio == wm.f32(0.2)
    db, err = DB.NewSimpleDB(str(tmp_path))
    assert err is None
    assert (db.compactionFileThreshold, db.compactedMaxSizeBytes, db.compactionRatio) == (10, 5 << 30, wm.f32(0.2))
    assert db.enableCompactions and not db.compactOnDevice and not db._compaction_active()
    db, err = DB.NewSimpleDB(str(tmp_path), DB.CompactionFileThreshold(3), DB.CompactionMaxSizeBytes(1234),
                             DB.CompactionRatio(0.5), DB.CompactionRunInterval(0.1), DB.CompactOnDevice())
    assert err is None
    assert (db.compactionFileThreshold, db.compactedMaxSizeBytes, db.compactionRatio) == (3, 1234, 0.5)
    assert db._compaction_active()
    db, _ = DB.NewSimpleDB(str(tmp_path), DB.CompactOnDevice(), DB.DisableCompactions())
    assert db.compactOnDevice and not db._compaction_active()
    db, _ = DB.NewSimpleDB(str(tmp_path), DB.CompactionRatio(0.1))
    assert db.compactionRatio == wm.f32(0.1)


@pytest.mark.parametrize("ratio", [1.5, -0.01, float("nan")])
def test_compaction_ratio_outside_0_1_raises(ratio):
    with pytest.raises(ValueError) as e:
        DB.CompactionRatio(ratio)
    assert str(e.value) == "invalid compaction ratio: %f, must be between 0 and 1" % ratio
    assert DB.CompactionRatio(0.0) and DB.CompactionRatio(1.0)


class _Reader:
    """What the selection reads of a reader; no table behind it."""

    def __init__(self, path, m):
        self.path, self.m = path, m

    def BasePath(self):  # noqa: N802
        return self.path

    def MetaData(self):  # noqa: N802
        return self.m


def test_execute_compacts_only_more_candidates_than_the_file_threshold(tmp_path):
    db, err = DB.NewSimpleDB(str(tmp_path), DB.CompactOnDevice(), DB.CompactionFileThreshold(3))
    assert err is None
    db.readers = [_Reader(str(tmp_path / (wm.TABLE_NAME % g)), meta(100, 10, 0)) for g in (1, 2, 3)]
    assert db._execute_compaction() == (None, None) and os.listdir(tmp_path) == []  # 3 <= 3: no write folder either
    # 3 > 2: a write folder is made, and the merge refuses readers that hold no table; the folder is removed again
    # and the readers stay as they were
    db.compactionFileThreshold = 2
    before = list(db.readers)
    m, err = db._execute_compaction()
    assert m is None and err is not None and os.listdir(tmp_path) == [] and db.readers == before
    db.compactedMaxSizeBytes = 100  # totalBytes < limit holds for none now
    assert db._execute_compaction() == (None, None)


def test_compact_before_open_is_not_opened_yet(tmp_path):
    for opts in ((), (DB.CompactOnDevice(),)):
        db, err = DB.NewSimpleDB(str(tmp_path), *opts)
        assert err is None
        assert db.Compact() == (None, DB.ErrNotOpenedYet)
