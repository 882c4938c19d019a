"""The write path's host side (CPU): the model's running size estimate (tests/db_write_model.py) against the host
MemStore after every op, the argument errors of rio_mem_size_scan that come back before any device call, and the DB
object's calls that need no device: NewSimpleDB on a missing directory, everything before Open."""
import ctypes
import random

import db_write_model as wm
import memstore as M
import simpledb as DB
from recordio import _lib as L


def seeded_ops(seed, n, n_keys=24, delete_share=0.3, value_lens=(0, 1, 7, 40, 300)):
    rng = random.Random(seed)
    keys = [b"", b"a", b"a\0", b"ab"] + [b"key%03d" % i for i in range(n_keys)]
    ops = []
    for _ in range(n):
        k = rng.choice(keys)
        if rng.random() < delete_share:
            ops.append((k, None))
        else:
            ops.append((k, bytes(rng.randrange(256) for _ in range(rng.choice(value_lens)))))
    return ops


def test_model_size_follows_the_host_memstore_after_every_op():
    for seed in (1, 2, 3):
        store = M.NewMemStore()
        rw = DB.RWMemstore(store, store)  # db.go:402: both halves are the one store until the first rotation
        model = wm.ModelMemStore()
        for i, (k, v) in enumerate(seeded_ops(seed, 700)):
            assert (rw.Delete(k) if v is None else rw.Upsert(k, v)) is None
            model.apply((k, v))
            assert model.size == store._size & wm.U64, (seed, i)
            assert model.estimated() == rw.EstimatedSizeInBytes(), (seed, i)


def test_float32_rule_of_the_estimate():
    """uint64(1.15 * float32(size)): the conversion rounds to nearest even, the product once more."""
    assert wm.u64_to_f32((1 << 24) + 1) == float(1 << 24) and wm.u64_to_f32((1 << 24) + 3) == float((1 << 24) + 4)
    assert wm.u64_to_f32((1 << 53) + 1 + (1 << 29)) == float((1 << 53) + (1 << 30))  # a double in between rounds down
    for size in (0, 1, 100, (1 << 24) + 1, (1 << 25) + 3, 1 << 32, (1 << 40) + (1 << 17)):
        assert wm.estimate(size) == int(M._f32(M._f32(1.15) * M._f32(float(size))))
    assert wm.estimate(100) == 115 and wm.estimate(1 << 32) == 4939212288


def test_size_scan_refuses_arguments_before_any_device_call():
    """RIO_ERR_ARG / RIO_ERR_UNSUPPORTED come back before the context or the device is touched: the calls are made
    with placeholder handles and device pointers on a machine that may have no GPU."""
    lib = L.lib()
    ctx, ptr = ctypes.c_void_p(8), ctypes.c_void_p(64)
    ops = L.OpsView(keys=64, key_off=64, values=64, val_off=64, flags=64, n=5, key_bytes=10, value_bytes=10)
    store = L.MemIndex(ops=ops, order=64, pfx=64, result=64)
    av = ctypes.addressof

    def scan(c=ctx, s=store, b=ops, max_key_len=8, size=ptr, res=ptr):
        return lib.rio_mem_size_scan(c, None if s is None else av(s), 0, None if b is None else av(b), max_key_len, 100,
                                     size, res, None)

    assert scan(c=None) == L.RIO_ERR_ARG
    assert scan(b=None) == L.RIO_ERR_ARG
    assert scan(res=None) == L.RIO_ERR_ARG
    assert scan(size=None) == L.RIO_ERR_ARG
    fields = {k: getattr(ops, k) for k, _ in L.OpsView._fields_}
    for field in ("keys", "key_off", "values", "val_off", "flags"):
        assert scan(b=L.OpsView(**dict(fields, **{field: None}))) == L.RIO_ERR_ARG, field
    # a store refused as by rio_mem_lookup
    assert scan(s=L.MemIndex(ops=ops, order=64, pfx=64, result=None)) == L.RIO_ERR_ARG
    assert scan(s=L.MemIndex(ops=ops, order=None, pfx=64, result=64)) == L.RIO_ERR_ARG
    assert scan(s=L.MemIndex(ops=ops, order=64, pfx=None, result=64)) == L.RIO_ERR_ARG
    assert scan(s=L.MemIndex(ops=L.OpsView(**dict(fields, keys=None)), order=64, pfx=64, result=64)) == L.RIO_ERR_ARG
    assert scan(s=L.MemIndex(ops=L.OpsView(**dict(fields, n=1 << 40)), order=64, pfx=64, result=64)) == L.RIO_ERR_UNSUPPORTED
    assert scan(max_key_len=L.RIO_FLUSH_MAX_KEY_LEN + 1) == L.RIO_ERR_UNSUPPORTED
    assert scan(b=L.OpsView(**dict(fields, n=(1 << 31) - 1))) == L.RIO_ERR_UNSUPPORTED
    assert scan(s=None, c=None) == L.RIO_ERR_ARG
    assert "rio_mem_size_scan" in L.EXPORTED
    assert (L.RIO_SIZE_R_CUT, L.RIO_SIZE_R_SIZE, L.RIO_SIZE_R_KEY_END, L.RIO_SIZE_R_VALUE_END, L.RIO_SIZE_R_FIRST_BAD) == \
        (0, 1, 2, 3, 4) and L.RIO_SIZE_RESULT_WORDS == 8


def test_new_simple_db_on_a_missing_directory_returns_its_error(tmp_path):
    missing = str(tmp_path / "nope")
    db, err = DB.NewSimpleDB(missing)
    assert db is None and str(err) == f"open {missing}: no such file or directory"
    db, err = DB.NewSimpleDB(str(tmp_path), DB.MemstoreSizeBytes(4096), DB.DisableCompactions())
    assert err is None and db.memstoreMaxSize == 4096 and db.enableCompactions is False
    assert DB.NewSimpleDB(str(tmp_path))[0].memstoreMaxSize == DB.MemStoreMaxSizeBytes == 1 << 30


def test_calls_before_open_give_err_not_opened_yet(tmp_path):
    db, err = DB.NewSimpleDB(str(tmp_path))
    assert err is None
    batch = DB.WriteBatch()
    batch.PutBytes(b"k", b"v")
    assert db.Apply(batch) is DB.ErrNotOpenedYet
    assert db.PutBytes(b"k", b"v") is DB.ErrNotOpenedYet and db.DeleteBytes(b"k") is DB.ErrNotOpenedYet
    assert db.Put("k", "v") is DB.ErrNotOpenedYet and db.Delete("k") is DB.ErrNotOpenedYet
    assert db.Put("", "v") is DB.ErrEmptyKeyValue and db.Put("k", "") is DB.ErrEmptyKeyValue  # db.go:245: checked first
    assert db.GetBytes(b"k") == (None, DB.ErrNotOpenedYet) and db.Get("k") == ("", DB.ErrNotOpenedYet)
    assert db.GetBatch([b"k", b"l"]) == [(None, DB.ErrNotOpenedYet)] * 2
    assert db.Close() is DB.ErrNotOpenedYet
    assert list(tmp_path.iterdir()) == []  # nothing was created
    assert str(DB.ErrNotOpenedYet) == "database has not been opened yet, please call Open() first"
    assert str(DB.ErrAlreadyOpen) == "database is already open" and str(DB.ErrAlreadyClosed) == "database is already closed"
    assert (DB.SSTablePrefix, DB.SSTablePattern, DB.WriteAheadFolder) == ("sstable", "sstable_%015d", "wal")
