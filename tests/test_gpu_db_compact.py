"""Compaction of simpledb.DB on the device (GPU), against the model of tests/db_compact_model.py. After every step the
directory is the model's: the same tables (names, Scan; index.rio and data.rio byte for byte with a table the host
MemStore flushes from the model's dict; meta.pb.bin by its fields; the bloom file by membership), a compacted table
with its compaction_successful record, the same WAL files and the same reads, resurrected values included. Then the
compacted table's resident install: the reader reflect makes from the merge's buffers against NewSSTableReader of the
same directory."""
import os
import random

import pytest

import db_compact_model as cm
import db_write_model as wm
import memstore as M
import simpledb as DB
import sstables as S
from recordio import _lib as L
from recordio.writer import encode_file
from sstables import proto as SP
from test_gpu_db import batch_of, same_reads, scan_table, seeded, wal_records

pytestmark = pytest.mark.gpu

FILES = (S.IndexFileName, S.DataFileName, S.MetaFileName, S.BloomFileName)
NEVER = 1000  # a file threshold no test reaches: only Compact() after the test lowers it compacts


def open_db(path, max_size, *opts, want=None):
    db, err = DB.NewSimpleDB(str(path), DB.MemstoreSizeBytes(max_size), DB.CompactOnDevice(), *opts)
    assert err is None, err
    assert db.Open() is want
    return db


def name_of(gen):
    return wm.TABLE_NAME % gen


def total_bytes(base, model):
    """{generation: totalBytes} as the tables' meta files have it."""
    out = {}
    for g, _ in model.tables:
        with open(os.path.join(str(base), name_of(g), S.MetaFileName), "rb") as fh:
            out[g] = SP.MetaData.unmarshal(fh.read()).totalBytes
    return out


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def same_directory(base, model, tmp_path, live=True):
    base = str(base)
    assert sorted(os.listdir(base)) == sorted([name_of(g) for g, _ in model.tables] + [DB.WriteAheadFolder])
    last = {rep: gens for rep, gens in model.compactions}  # a replacement's latest compaction
    for gen, table in model.tables:
        path = os.path.join(base, name_of(gen))
        compacted = gen in last
        reader, got = scan_table(path)
        assert got == sorted(table.items()), gen
        if table:
            ms = M.NewMemStore()
            for k, v in table.items():
                assert (ms.Tombstone(k) if v is None else ms.Upsert(k, v)) is None
            ref = str(tmp_path / f"ref_{os.path.basename(base)}_{gen}")
            assert (ms.Flush if compacted else ms.FlushWithTombstones)(S.WriteBasePath(ref)) is None
            for name in (S.IndexFileName, S.DataFileName):
                assert read(os.path.join(path, name)) == read(os.path.join(ref, name)), (gen, name)
        else:  # a compaction without survivors: two files of a header alone
            assert compacted
            assert read(os.path.join(path, S.IndexFileName)) == encode_file([], L.COMP_NONE)
            assert read(os.path.join(path, S.DataFileName)) == encode_file([], L.COMP_SNAPPY)
        meta = reader.MetaData()
        assert SP.MetaData.unmarshal(read(os.path.join(path, S.MetaFileName))) == meta
        nd, ni = (os.path.getsize(os.path.join(path, n)) for n in (S.DataFileName, S.IndexFileName))
        assert (meta.version, meta.numRecords, meta.dataBytes, meta.indexBytes, meta.totalBytes) == (1, len(table), nd, ni, nd + ni)
        assert meta.nullValues == (0 if compacted else sum(1 for v in table.values() if v is None))
        assert (meta.minKey, meta.maxKey) == ((min(table), max(table)) if table else (b"", b""))
        flt = reader.bloomFilter
        assert flt is not None and all(flt.Contains(k) for k in table)
        if compacted:
            assert sorted(os.listdir(path)) == sorted(FILES + (DB.CompactionFinishedSuccessfulFileName,))
            m, err = DB.read_compaction_metadata(os.path.join(path, DB.CompactionFinishedSuccessfulFileName))
            assert err is None, err
            assert m.writePath.startswith(DB.SSTableCompactionPathPrefix) and len(m.writePath) > len(DB.SSTableCompactionPathPrefix)
            assert m.replacementPath == name_of(gen) and m.sstablePaths == [name_of(g) for g in last[gen]]
        else:
            assert sorted(os.listdir(path)) == sorted(FILES)
        assert reader.Close() is None
    wal_dir = os.path.join(base, DB.WriteAheadFolder)
    assert sorted(os.listdir(wal_dir)) == sorted(model.wal)
    for name, ops in model.wal.items():
        if not (live and name == max(model.wal)):
            assert wal_records(os.path.join(wal_dir, name)) == ops, name


def same_stack(db, model):
    assert [os.path.basename(r.BasePath()) for r in db.readers] == [name_of(g) for g, _ in model.tables]


def compact_both(db, model, base, threshold, max_size, ratio):
    """One Compact() with these settings (for this call alone: the writes after it trigger no pass) next to the
    model's pass over the tables' own totalBytes -> the generations."""
    gens = model.compact(total_bytes(base, model), threshold, max_size, ratio)
    generation = db.currentGeneration
    before = db.compactionFileThreshold, db.compactedMaxSizeBytes, db.compactionRatio
    db.compactionFileThreshold, db.compactedMaxSizeBytes, db.compactionRatio = threshold, max_size, wm.f32(ratio)
    try:
        m, err = db.Compact()
    finally:
        db.compactionFileThreshold, db.compactedMaxSizeBytes, db.compactionRatio = before
    assert err is None, err
    assert db.currentGeneration == generation
    if gens is None:
        assert m is None
    else:
        assert (m.replacementPath, m.sstablePaths) == (name_of(gens[0]), [name_of(g) for g in gens])
    same_stack(db, model)
    return gens


# ---- automatic passes ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("threshold, max_size", [(1, 200), (3, 300), (2, 600)])
def test_automatic_passes_leave_the_models_directory(tmp_path, threshold, max_size):
    base = tmp_path / "db"
    base.mkdir()
    db = open_db(base, max_size, DB.CompactionFileThreshold(threshold))
    model = cm.ModelCompactDB(max_size, threshold)
    same_directory(base, model, tmp_path)
    for seed, n in ((1, 300), (2, 1), (3, 150)):
        ops = seeded(seed, n)
        assert db.Apply(batch_of(ops)) is None
        model.apply(ops)
        same_directory(base, model, tmp_path)
        same_stack(db, model)
        same_reads(db, model, extra=[k for k, _ in ops])
    assert len(model.compactions) >= 2 and len(model.tables) <= threshold + 1
    assert db.currentGeneration == model.generation > len(model.tables)
    assert db.Close() is None
    model.close()
    same_directory(base, model, tmp_path, live=False)


def test_disable_compactions_after_the_opt_in_runs_nothing(tmp_path):
    base = tmp_path / "db"
    base.mkdir()
    db = open_db(base, 200, DB.CompactionFileThreshold(1), DB.DisableCompactions())
    model = cm.ModelCompactDB(200)  # no threshold: no pass
    ops = seeded(4, 100)
    assert db.Apply(batch_of(ops)) is None
    model.apply(ops)
    assert len(model.tables) >= 4 and not model.compactions
    assert db.Compact() == (None, None)
    same_directory(base, model, tmp_path)
    same_reads(db, model)
    assert db.Close() is None
    # without the opt-in Compact() is refused, and the default options compact nothing either
    db, err = DB.NewSimpleDB(str(base), DB.MemstoreSizeBytes(200), DB.CompactionFileThreshold(1))
    assert err is None and db.Open() is None
    m, err = db.Compact()
    assert m is None and isinstance(err, S.UnsupportedError)
    model.close()
    model.reopen()
    same_directory(base, model, tmp_path)
    assert db.Close() is None


# ---- Compact() on demand -----------------------------------------------------------------------------------------

def big(seed, n):
    rng = random.Random(seed)
    return bytes(rng.randrange(256) for _ in range(n))  # does not compress


def test_flood_fill_takes_a_middle_table_over_the_size_limit(tmp_path):
    base = tmp_path / "db"
    base.mkdir()
    db, model = open_db(base, 400, DB.CompactionFileThreshold(NEVER)), cm.ModelCompactDB(400)
    # two small tables, one that a single large value makes large, two small ones
    for ops in (seeded(11, 120), [(b"key005", big(1, 3000))], seeded(12, 120)):
        assert db.Apply(batch_of(ops)) is None
        model.apply(ops)
    tb = total_bytes(base, model)
    gens = [g for g, _ in model.tables]
    largest = max(tb, key=tb.get)
    limit = tb[largest]
    assert len(gens) >= 5 and gens[0] != largest != gens[-1] and sorted(tb.values())[-2] < limit
    own = [cm.selected(tb[g], len(t), sum(v is None for v in t.values()), limit, 1.0) for g, t in model.tables]
    assert own == [g != largest for g in gens]  # the size limit alone leaves the middle table out
    assert compact_both(db, model, base, 1, limit, 1.0) == gens
    assert len(model.tables) == 1
    same_directory(base, model, tmp_path)
    same_reads(db, model)
    assert compact_both(db, model, base, 1, limit, 1.0) is None  # one candidate is not more than the threshold
    assert db.Close() is None


def test_a_run_that_does_not_start_at_the_oldest_table_brings_hidden_values_back(tmp_path):
    base = tmp_path / "db"
    base.mkdir()
    db, model = open_db(base, 300, DB.CompactionFileThreshold(NEVER)), cm.ModelCompactDB(300)
    first = [(b"old%03d" % i, b"value%03d" % i) for i in range(8)] + [(b"large", big(2, 3000))]
    later = [(b"old%03d" % i, None) for i in range(0, 8, 2)] + seeded(13, 150, n_keys=40)
    for ops in (first, later, [(b"filler", big(3, 400))]):
        assert db.Apply(batch_of(ops)) is None
        model.apply(ops)
    gens = [g for g, _ in model.tables]
    tb = total_bytes(base, model)
    assert len(gens) >= 3 and max(tb, key=tb.get) == gens[0]
    hidden = [k for k, _ in first if model.get(k) is None]
    assert hidden  # tombstoned in a later table
    same_reads(db, model, extra=[k for k, _ in first])
    assert compact_both(db, model, base, 1, tb[gens[0]], 1.0) == gens[1:]
    assert [g for g, _ in model.tables] == gens[:2]
    # the reference's reducer drops the tombstones although an older table is left: its values are read again
    assert [model.get(k) for k in hidden] == [dict(first)[k] for k in hidden]
    same_directory(base, model, tmp_path)
    same_reads(db, model, extra=[k for k, _ in first])
    assert db.Close() is None


def test_the_tombstone_ratio_selects_tables_the_size_limit_leaves_out(tmp_path):
    base = tmp_path / "db"
    base.mkdir()
    db, model = open_db(base, 300, DB.CompactionFileThreshold(NEVER)), cm.ModelCompactDB(300)
    puts = [(b"put%03d" % i, b"v" * 30) for i in range(40)]
    for ops in (puts[:20], seeded(14, 200, replayable=True), puts[20:]):
        assert db.Apply(batch_of(ops)) is None
        model.apply(ops)
    gens = [g for g, _ in model.tables]
    own = [cm.selected(1, len(t), sum(v is None for v in t.values()), 0, cm.DEFAULT_RATIO) for _, t in model.tables]
    assert not own[0] and not own[-1] and sum(own) >= 2  # tables of puts alone at both ends
    want = gens[own.index(True):len(own) - own[::-1].index(True)]
    assert compact_both(db, model, base, 1, 0, cm.DEFAULT_RATIO) == want
    same_directory(base, model, tmp_path)
    same_reads(db, model)
    assert db.Close() is None


def test_a_run_without_survivors_leaves_an_empty_table(tmp_path):
    base = tmp_path / "db"
    base.mkdir()
    db, model = open_db(base, 200, DB.CompactionFileThreshold(NEVER)), cm.ModelCompactDB(200)
    keys = [b"gone%03d" % i for i in range(30)]
    # the puts rotate several times; the deletes never do (db.go:311-347), the put of an empty value after them does
    for ops in ([(k, b"value of " + k) for k in keys], [(k, None) for k in keys] + [(b"empty", b"")]):
        assert db.Apply(batch_of(ops)) is None
        model.apply(ops)
    gens = [g for g, _ in model.tables]
    assert len(gens) >= 3 and not model.mem.latest
    assert compact_both(db, model, base, 1, 1 << 40, 1.0) == gens
    assert model.tables == [(1, {})]
    same_directory(base, model, tmp_path)
    same_reads(db, model, extra=keys)
    # the empty table is a candidate like any other, and its reader serves the stack
    more = seeded(15, 120)
    assert db.Apply(batch_of(more)) is None
    model.apply(more)
    same_reads(db, model, extra=keys)
    gens = [g for g, _ in model.tables]
    assert len(gens) >= 3 and compact_both(db, model, base, 1, 1 << 40, 1.0) == gens
    same_directory(base, model, tmp_path)
    same_reads(db, model, extra=keys)
    assert db.Close() is None


# ---- Close, reopen, and the protocol interrupted -------------------------------------------------------------------

def test_reopen_counts_generations_from_the_highest_remaining_suffix(tmp_path):
    base = tmp_path / "db"
    base.mkdir()
    db, model = open_db(base, 300, DB.CompactionFileThreshold(1)), cm.ModelCompactDB(300, 1)
    ops = seeded(16, 250, replayable=True) + [(b"last", big(5, 400))]  # the last put rotates: the memstore is empty
    assert db.Apply(batch_of(ops)) is None
    model.apply(ops)
    assert [g for g, _ in model.tables] == [1] and model.generation >= 4 and not model.mem.latest
    assert db.currentGeneration == model.generation
    assert db.Close() is None
    model.close()
    same_directory(base, model, tmp_path, live=False)
    db = open_db(base, 300, DB.CompactionFileThreshold(1))
    model.reopen()
    assert db.currentGeneration == model.generation == 1
    same_directory(base, model, tmp_path)
    same_reads(db, model, extra=[k for k, _ in ops])
    more = seeded(17, 60, replayable=True) + [(b"last", big(6, 400))]
    assert db.Apply(batch_of(more)) is None
    model.apply(more)
    same_directory(base, model, tmp_path)
    same_reads(db, model, extra=[k for k, _ in ops])
    assert db.Close() is None


def test_open_finishes_a_compaction_that_was_executed_and_not_reflected(tmp_path):
    base = tmp_path / "db"
    base.mkdir()
    db, model = open_db(base, 300, DB.CompactionFileThreshold(NEVER)), cm.ModelCompactDB(300)
    ops = seeded(18, 250, replayable=True)
    assert db.Apply(batch_of(ops)) is None
    model.apply(ops)
    assert len(model.tables) >= 3 and model.mem.latest
    db.compactionFileThreshold = 1
    m, err = db._execute_compaction()
    assert err is None and m.sstablePaths == [name_of(g) for g, _ in model.tables]
    assert sorted(os.listdir(base / m.writePath)) == sorted(FILES + (DB.CompactionFinishedSuccessfulFileName,))
    assert db.wal.Close() is None  # the process ends here: the write folder and every input are on disk
    listing = lambda: sorted((str(p.relative_to(base)), p.stat().st_size) for p in base.rglob("*"))  # noqa: E731
    before = listing()
    # without the opt-in the database stays with the reference, untouched
    plain, err = DB.NewSimpleDB(str(base), DB.MemstoreSizeBytes(300))
    assert err is None and isinstance(plain.Open(), S.UnsupportedError) and listing() == before
    disabled, err = DB.NewSimpleDB(str(base), DB.CompactOnDevice(), DB.DisableCompactions())
    assert err is None and isinstance(disabled.Open(), S.UnsupportedError) and listing() == before
    db = open_db(base, 300, DB.CompactionFileThreshold(NEVER))
    model.reopen(repair=({}, 1, cm.DEFAULT_MAX_SIZE, cm.DEFAULT_RATIO))  # every table is far below the size limit
    assert [g for g, _ in model.tables] == [1, 2] and db.currentGeneration == 2
    same_directory(base, model, tmp_path)
    same_stack(db, model)
    same_reads(db, model, extra=[k for k, _ in ops])
    assert db.Close() is None


# ---- the compacted table enters the stack from the merge's buffers -------------------------------------------------

def scan(it_err):
    it, err = it_err
    assert err is None, err
    out = []
    while True:
        k, v, err = it.Next()
        if err is S.Done:
            return out
        assert err is None, err
        out.append((k, v))


@pytest.mark.parametrize("seed", [21, 22, 23])
def test_the_installed_reader_equals_a_reader_loaded_from_the_files(tmp_path, seed):
    base = tmp_path / "db"
    base.mkdir()
    db, model = open_db(base, 300, DB.CompactionFileThreshold(NEVER)), cm.ModelCompactDB(300)
    ops = seeded(seed, 200) + [(b"long", big(seed, 3000))] + seeded(seed + 100, 100)
    assert db.Apply(batch_of(ops)) is None
    model.apply(ops)
    gens = [g for g, _ in model.tables]
    assert compact_both(db, model, base, 1, 1 << 40, 1.0) == gens
    a = db.readers[0]
    b, err = S.NewSSTableReader(S.ReadBasePath(a.BasePath()), S.ReadOnDevice(db.device))
    assert err is None, err
    ta, tb = a.t, b.t
    n = tb.n_index
    assert n == len(model.tables[0][1]) > 0
    for name in ("n_index", "n_data", "index_bad", "value_bad", "bad_proto", "bad_crc", "unplaced", "v0", "index_img", "data_img",
                 "h_key_off", "h_key_len", "h_value_off", "h_checksum", "h_crc", "h_index", "h_data", "h_data_off",
                 "h_data_flags", "h_view"):
        assert getattr(ta, name) == getattr(tb, name), name
    for name in ("version", "compression", "n_records", "total_out_bytes", "status", "n_bad"):
        assert ta.index_info[name] == tb.index_info[name] and ta.data_info[name] == tb.data_info[name], name
    nb_i, nb_d = tb.index_info["total_out_bytes"], tb.data_info["total_out_bytes"]
    for name in ("key_off", "key_len", "value_off", "checksum", "crc"):
        assert getattr(ta, name)[:n].cpu().tolist() == getattr(tb, name)[:n].cpu().tolist(), name
    for buf, nbytes in (("ib", nb_i), ("db", nb_d)):
        x, y = getattr(ta, buf), getattr(tb, buf)
        assert bytes(x.out[:nbytes].cpu().numpy()) == bytes(y.out[:nbytes].cpu().numpy()), buf
        assert x.out_off[:n + 1].cpu().tolist() == y.out_off[:n + 1].cpu().tolist(), buf
        assert x.rec_off[:n].cpu().tolist() == y.rec_off[:n].cpu().tolist(), buf
        assert x.flags[:n].cpu().tolist() == y.flags[:n].cpu().tolist(), buf
    assert a.MetaData() == b.MetaData() and a.MetaData().marshal() == b.MetaData().marshal()
    fa, fb = a.bloomFilter, b.bloomFilter
    assert (fa.m, fa.k, list(fa.keys), bytes(fa.bits), fa.N()) == (fb.m, fb.k, list(fb.keys), bytes(fb.bits), fb.N())
    table = model.tables[0][1]
    keys = sorted(table) + [b"absent", b"", b"key", b"zzz"]
    assert a.GetBatch(keys) == b.GetBatch(keys) == [(table[k], None) if k in table else (None, S.NotFound) for k in keys]
    assert a.ContainsBatch(keys) == b.ContainsBatch(keys) == [(k in table, None) for k in keys]
    assert [a.Get(k) for k in keys[::5]] == [b.Get(k) for k in keys[::5]]
    assert scan(a.Scan()) == scan(b.Scan()) == sorted(table.items())
    for lo in (b"", b"key010", b"key0100", b"zzzz"):
        assert scan(a.ScanStartingAt(lo)) == scan(b.ScanStartingAt(lo)) == sorted((k, v) for k, v in table.items() if k >= lo)
    for lo, hi in ((b"a", b"key020"), (b"key005", b"key005"), (b"", b"\xff"), (b"x", b"y")):
        assert scan(a.ScanRange(lo, hi)) == scan(b.ScanRange(lo, hi)) == sorted((k, v) for k, v in table.items() if lo <= k <= hi)
    # a stack over the reader loaded from the files answers what the DB's stack over the installed one answers
    other = DB.DBReadView(S.NewSuperSSTableReader([b]), db.memStore)
    assert db.GetBatch(keys) == other.GetBatch(keys)
    same_reads(db, model, extra=[k for k, _ in ops])
    assert other.Close() is None and b.Close() is None
    assert db.Close() is None


def test_reflect_reads_no_file_and_a_forced_reload_gives_the_same_database(tmp_path, monkeypatch):
    ops = seeded(24, 300)
    dbs = []
    for name, install in (("hbm", True), ("reload", False)):
        base = tmp_path / name
        base.mkdir()
        db, model = open_db(base, 300, DB.CompactionFileThreshold(NEVER)), cm.ModelCompactDB(300)
        assert db.Apply(batch_of(ops)) is None
        model.apply(ops)
        db.installCompactedFromDevice = install
        if install:
            def refuse(*options):
                raise AssertionError("reflect loaded the compacted table from its files")

            with monkeypatch.context() as mp:
                mp.setattr(S, "NewSSTableReader", refuse)
                assert compact_both(db, model, base, 1, 1 << 40, 1.0) is not None
        else:
            assert compact_both(db, model, base, 1, 1 << 40, 1.0) is not None
        same_directory(base, model, tmp_path)
        same_reads(db, model, extra=[k for k, _ in ops])
        dbs.append(db)
    keys = sorted({k for k, _ in ops})
    assert dbs[0].GetBatch(keys) == dbs[1].GetBatch(keys)
    for name in (S.IndexFileName, S.DataFileName, S.MetaFileName):
        assert read(tmp_path / "hbm" / name_of(1) / name) == read(tmp_path / "reload" / name_of(1) / name)
    for db in dbs:
        assert db.Close() is None
