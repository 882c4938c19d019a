"""simpledb.DB on the device (GPU): NewSimpleDB / Open / Apply / Put / Get / Close against the sequential model
(tests/db_write_model.py). Small MemstoreSizeBytes values make a few hundred ops rotate several times. After every
step the directory is the model's: the same tables (names, Scan, and index.rio / data.rio / meta.pb.bin byte for byte
with a table the host MemStore flushes from the model's dict; the bloom file by membership, its hash keys are
random), the same WAL files with the same decoded records, and the same reads."""
import os
import random

import pytest

import db_write_model as wm
import memstore as M
import recordio as R
import simpledb as DB
import sstables as S
from recordio import _lib as L
from recordio.errors import EOF, errors_is
from simpledb import proto

pytestmark = pytest.mark.gpu

FILES = (S.IndexFileName, S.DataFileName, S.MetaFileName)


def batch_of(ops):
    b = DB.WriteBatch()
    for k, v in ops:
        assert (b.DeleteBytes(k) if v is None else b.PutBytes(k, v)) is None
    return b


def seeded(seed, n, n_keys=60, replayable=False, long=1):
    """replayable: no empty key and no empty value. The reference's replay reads an addition without keyBytes or
    valueBytes through its string fields or as Upsert(key, nil) (recovery.go:224-230), so such a WAL does not
    recover to what was written. long: the longest values' length in units of 40 bytes."""
    rng = random.Random(seed)
    keys = ([] if replayable else [b""]) + [b"a", b"a\0", b"prefix_8a", b"prefix_8b"] + [b"key%03d" % i for i in range(n_keys)]
    lens = (1, 8, 40) if replayable else (0, 1, 8, 40 * long)
    ops = []
    for _ in range(n):
        k = rng.choice(keys)
        ops.append((k, None) if rng.random() < 0.25 else (k, bytes(rng.randrange(256) for _ in range(rng.choice(lens)))))
    return ops


def open_db(path, max_size):
    db, err = DB.NewSimpleDB(str(path), DB.MemstoreSizeBytes(max_size), DB.DisableCompactions())
    assert err is None, err
    assert db.Open() is None
    return db


def wal_records(path):
    """The decoded ops of one WAL file."""
    r, err = R.NewFileReaderWithPath(path)
    assert err is None, err
    assert r.Open() is None
    out = []
    while True:
        rec, err = r.ReadNext()
        if errors_is(err, EOF):
            break
        assert err is None, err
        m = proto.unmarshal_wal_mutation(rec)  # what PutBytes / DeleteBytes marshalled: the bytes fields alone
        assert m.member in (proto.ADDITION, proto.DELETE_TOMBSTONE) and not m.key and not m.value
        out.append((m.keyBytes, m.valueBytes if m.member == proto.ADDITION else None))
    r.Close()
    return out


def scan_table(path):
    r, err = S.NewSSTableReader(S.ReadBasePath(path))
    assert err is None, err
    it, err = r.Scan()
    assert err is None, err
    out = []
    while True:
        k, v, err = it.Next()
        if err is S.Done:
            break
        assert err is None, err
        out.append((k, v))
    return r, out


def same_directory(base, model, tmp_path, live=True):
    """The directory under `base` is the model's. live: a DB has the newest WAL file open, and its writer holds the
    file's bytes until it closes: that file's records are compared once it is closed (live=False)."""
    base = str(base)
    names = sorted(os.listdir(base))
    assert names == sorted([wm.TABLE_NAME % g for g, _ in model.tables] + [DB.WriteAheadFolder])
    for gen, table in model.tables:
        path = os.path.join(base, wm.TABLE_NAME % gen)
        reader, got = scan_table(path)
        assert got == sorted(table.items()), gen
        # the table the host MemStore flushes from the same dict
        ms = M.NewMemStore()
        for k, v in table.items():
            assert (ms.Tombstone(k) if v is None else ms.Upsert(k, v)) is None
        ref = str(tmp_path / f"ref_{os.path.basename(base)}_{gen}")
        assert ms.FlushWithTombstones(S.WriteBasePath(ref)) is None
        for name in FILES:
            with open(os.path.join(path, name), "rb") as a, open(os.path.join(ref, name), "rb") as b:
                assert a.read() == b.read(), (gen, name)
        assert sorted(os.listdir(path)) == sorted(FILES + (S.BloomFileName,))
        flt = reader.bloomFilter
        assert flt is not None and all(flt.Contains(k) for k in table)
        assert reader.Close() is None
    wal_dir = os.path.join(base, DB.WriteAheadFolder)
    assert sorted(os.listdir(wal_dir)) == sorted(model.wal)
    for name, ops in model.wal.items():
        if not (live and name == max(model.wal)):
            assert wal_records(os.path.join(wal_dir, name)) == ops, name
    assert max(model.max_wal_bytes, model.raw_wal_bytes()) < model.max_size * 50  # the model's premise: the WAL's own limit is never reached


def same_reads(db, model, extra=()):
    keys = sorted({k for _, t in model.tables for k in t} | set(model.mem.latest) | set(extra)) + [b"never written"]
    want = [(model.get(k), None) if model.get(k) is not None else (None, DB.ErrNotFound) for k in keys]
    assert db.GetBatch(keys) == want
    for k in keys[::7]:
        assert db.GetBytes(k) == (model.get(k), None if model.get(k) is not None else DB.ErrNotFound)


@pytest.mark.parametrize("max_size", [200, 1000, 4096])
def test_apply_leaves_the_models_directory(tmp_path, max_size):
    base = tmp_path / "db"
    base.mkdir()
    db, model = open_db(base, max_size), wm.ModelDB(max_size)
    same_directory(base, model, tmp_path)
    for seed, n in ((1, 300), (2, 1), (3, 150)):
        ops = seeded(seed, n, long=10 if max_size == 4096 else 1)  # longer values fill the largest memstore too
        assert db.Apply(batch_of(ops)) is None
        model.apply(ops)
        same_directory(base, model, tmp_path)
        same_reads(db, model)
    assert len(model.tables) >= 3
    assert db.Close() is None
    model.close()
    same_directory(base, model, tmp_path, live=False)


def test_one_batch_single_calls_and_batches_of_7_leave_the_same_directory(tmp_path):
    ops = seeded(5, 180, n_keys=30)
    model = wm.ModelDB(300)
    model.apply(ops)
    assert len(model.tables) >= 3

    def apply_whole(db):
        assert db.Apply(batch_of(ops)) is None

    def apply_singly(db):
        for k, v in ops:
            assert (db.DeleteBytes(k) if v is None else db.PutBytes(k, v)) is None

    def apply_by_7(db):
        for a in range(0, len(ops), 7):
            assert db.Apply(batch_of(ops[a:a + 7])) is None

    for name, run in (("whole", apply_whole), ("singly", apply_singly), ("by7", apply_by_7)):
        base = tmp_path / name
        base.mkdir()
        db = open_db(base, 300)
        run(db)
        same_directory(base, model, tmp_path)
        same_reads(db, model)
        assert db.wal.Close() is None  # the process ends here: the newest WAL file holds the memstore's ops
        same_directory(base, model, tmp_path, live=False)


def test_put_get_delete_strings(tmp_path):
    db = open_db(tmp_path, 4096)
    assert db.Put("", "v") is DB.ErrEmptyKeyValue and db.Put("k", "") is DB.ErrEmptyKeyValue
    assert db.Put("hello", "world") is None and db.Get("hello") == ("world", None)
    assert db.Put("hello", "again") is None and db.Get("hello") == ("again", None)
    assert db.Delete("hello") is None and db.Get("hello") == ("", DB.ErrNotFound)
    assert db.Get("absent") == ("", DB.ErrNotFound) and db.Delete("absent") is None
    assert db.memStore.EstimatedSizeInBytes() == wm.estimate(5 + 6)  # two tombstones: their keys' lengths
    # the batch on the device: the write store's value, its tombstone, an absent key
    assert db.PutBytes(b"kept", b"value") is None
    d_keys, d_off, _ = M.upload_queries(0, [b"kept", b"hello", b"nowhere"])
    mem, tab, status, val_off, values = db.GetBatchOnDevice(d_keys, d_off, 3)
    assert tab is None and status.cpu().tolist() == [L.RIO_GET_MEM_VALUE, L.RIO_GET_NOT_FOUND, L.RIO_GET_NOT_FOUND]
    assert val_off.cpu().tolist() == [0, 5, 5, 5] and bytes(values.cpu().numpy()) == b"value"
    assert db.Close() is None


def test_close_and_reopen_answers_the_same_reads(tmp_path):
    base = tmp_path / "db"
    base.mkdir()
    db, model = open_db(base, 500), wm.ModelDB(500)
    ops = seeded(7, 250)
    assert db.Apply(batch_of(ops)) is None
    model.apply(ops)
    assert db.Close() is None
    model.close()
    same_directory(base, model, tmp_path, live=False)
    db = open_db(base, 500)
    model.reopen()
    same_directory(base, model, tmp_path)
    same_reads(db, model, extra=[k for k, _ in ops])
    more = seeded(8, 120)
    assert db.Apply(batch_of(more)) is None
    model.apply(more)
    same_directory(base, model, tmp_path)
    same_reads(db, model, extra=[k for k, _ in ops])
    assert db.Close() is None


def test_a_wal_left_by_an_unclosed_db_recovers_to_the_same_reads(tmp_path):
    base = tmp_path / "db"
    base.mkdir()
    db, model = open_db(base, 400), wm.ModelDB(400)
    ops = seeded(9, 200, replayable=True)
    assert db.Apply(batch_of(ops)) is None
    model.apply(ops)
    assert model.mem.latest and len(model.tables) >= 2  # ops in the memstore that only the WAL holds
    before = [model.get(k) for k, _ in ops]
    assert db.wal.Close() is None  # the process ends here: no Close of the DB, the WAL file is complete
    same_directory(base, model, tmp_path, live=False)
    db = open_db(base, 400)
    model.reopen()
    assert [model.get(k) for k, _ in ops] == before
    same_directory(base, model, tmp_path)
    same_reads(db, model, extra=[k for k, _ in ops])
    assert db.Close() is None


def test_open_and_close_errors(tmp_path):
    db, err = DB.NewSimpleDB(str(tmp_path))
    assert err is None and db.Open() is None
    assert db.Open() is DB.ErrAlreadyOpen
    assert db.PutBytes(b"k", b"v") is None
    assert db.Close() is None
    assert db.Close() is DB.ErrAlreadyClosed
    assert db.Open() is DB.ErrAlreadyOpen  # db.go:120: open stays set
    assert db.PutBytes(b"k", b"v") is DB.ErrAlreadyClosed and db.DeleteBytes(b"k") is DB.ErrAlreadyClosed
    assert db.Apply(batch_of([(b"k", b"v")])) is DB.ErrAlreadyClosed
    assert db.GetBytes(b"k") == (None, DB.ErrAlreadyClosed) and db.Get("k") == ("", DB.ErrAlreadyClosed)
    assert db.GetBatch([b"k"]) == [(None, DB.ErrAlreadyClosed)]
    # the closed database holds the put in its one table, and the fresh header-only WAL file stays
    assert sorted(os.listdir(tmp_path)) == [wm.TABLE_NAME % 1, DB.WriteAheadFolder]
    assert os.listdir(tmp_path / DB.WriteAheadFolder) == [wm.WAL_NAME % 1]
    assert os.path.getsize(tmp_path / DB.WriteAheadFolder / (wm.WAL_NAME % 1)) == 8


def test_a_key_the_device_cannot_order_is_refused_before_anything_is_written(tmp_path):
    db = open_db(tmp_path, 4096)
    err = db.Apply(batch_of([(b"k", b"v"), (b"K" * (L.RIO_FLUSH_MAX_KEY_LEN + 1), b"v")]))
    assert isinstance(err, S.UnsupportedError)
    assert db.GetBytes(b"k") == (None, DB.ErrNotFound)
    assert db.Close() is None
    # no table, and both WAL files (the one Close rotated away from an empty memstore stays) hold their header alone
    assert sorted(os.listdir(tmp_path)) == [DB.WriteAheadFolder]
    wal_dir = tmp_path / DB.WriteAheadFolder
    assert sorted(os.listdir(wal_dir)) == [wm.WAL_NAME % 0, wm.WAL_NAME % 1]
    assert [os.path.getsize(wal_dir / name) for name in os.listdir(wal_dir)] == [8, 8]


def test_a_compaction_directory_is_left_to_the_reference(tmp_path):
    (tmp_path / "sstable_000000000000001").mkdir()
    (tmp_path / "sstable_compaction").mkdir()
    (tmp_path / "sstable_compaction" / "marker").write_bytes(b"x")
    before = sorted(str(p.relative_to(tmp_path)) for p in tmp_path.rglob("*"))
    db, err = DB.NewSimpleDB(str(tmp_path))
    assert err is None
    assert isinstance(db.Open(), S.UnsupportedError)
    assert sorted(str(p.relative_to(tmp_path)) for p in tmp_path.rglob("*")) == before
    assert db.GetBytes(b"k") == (None, DB.ErrNotOpenedYet)
