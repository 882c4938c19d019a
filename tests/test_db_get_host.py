"""The read path's host side (CPU): RWMemstore and MemStore point semantics against the model (tests/db_model.py) on
a seeded op sequence, DBReadView.GetBytes over stand-in tables, and the argument errors of rio_mem_index_build,
rio_mem_lookup and rio_db_* that come back before any device call."""
import ctypes
import random

import db_model as dm
import memstore as M
import simpledb as DB
import sstables as S
from recordio import _lib as L


def _err(e):
    """A store's error as the model names it."""
    return None if e is None else str(e)


def _apply(rng, stores, models, keys):
    """One random mutating call on the write store (through RWMemstore) and on its model."""
    rw, (w_model, _) = stores, models
    key = rng.choice(keys)
    kind = rng.randrange(4)
    if kind == 0:
        value = bytes(rng.randrange(256) for _ in range(rng.choice([0, 1, 5, 40])))
        assert rw.Upsert(key, value) is None
        w_model.upsert(key, value)
    elif kind == 1:
        # RWMemstore.Delete: the write store's KeyNotFound becomes a tombstone (rw_memstore.go:48-55)
        assert rw.Delete(key) is None
        if w_model.delete(key) == dm.KEY_NOT_FOUND:
            w_model.tombstone(key)
    elif kind == 2:
        assert rw.Tombstone(key) is None
        w_model.tombstone(key)
    else:
        assert _err(rw.writeStore.Delete(key)) == w_model.delete(key)


def test_rw_memstore_and_memstore_follow_the_model():
    rng = random.Random(5)
    keys = [b"", b"a", b"a\0", b"ab"] + [b"key%03d" % i for i in range(40)]
    read, r_model = M.NewMemStore(), dm.ModelStore()
    for _ in range(120):  # the store being flushed: filled before the pair exists
        key = rng.choice(keys)
        if rng.randrange(3):
            value = b"r" * rng.randrange(6)
            assert read.Upsert(key, value) is None
            r_model.upsert(key, value)
        else:
            assert read.Tombstone(key) is None
            r_model.tombstone(key)
    write, w_model = M.NewMemStore(), dm.ModelStore()
    rw = DB.RWMemstore(read, write)
    for step in range(600):
        _apply(rng, rw, (w_model, r_model), keys)
        if step % 50 == 49:
            for k in keys:
                v, e = rw.Get(k)
                assert (v, _err(e)) == dm.rw_get(w_model, r_model, k), k
                assert rw.Contains(k) == dm.rw_contains(w_model, r_model, k)
                assert (write.Get(k)[0], _err(write.Get(k)[1])) == w_model.get(k)
    # the sentinels themselves come back, and only the write store's KeyNotFound asks the read store
    never = b"never written"
    assert rw.Get(never) == (None, M.KeyNotFound) and rw.Get(never)[1] is M.KeyNotFound
    assert write.Tombstone(b"both") is None and read.Upsert(b"both", b"old") is None
    assert rw.Get(b"both")[1] is M.KeyTombstoned and not rw.Contains(b"only-read")
    assert rw.Size() == write.Size() and rw.EstimatedSizeInBytes() == write.EstimatedSizeInBytes()
    assert len(write._flags) == len(w_model.ops) + 1  # the log holds every accepted op, in order


class _Tables:
    """What DBReadView's host sequence needs of a table stack: Get by the newest dict that holds the key."""

    def __init__(self, tables, fail=None):
        self.tables, self.fail, self.max_batch = tables, fail or {}, 1 << 20

    def Get(self, key):  # noqa: N802
        if key in self.fail:
            return None, self.fail[key]
        v, err = dm.tables_get(self.tables, key)
        return (None, S.NotFound) if err is not None else (v, None)


def test_get_bytes_host_sequence_follows_db_go():
    tables = [{b"t": b"old", b"empty": b"", b"nil": None, b"both": b"table", b"dead": b"table", b"bad": b"x"},
              {b"t": b"new"}]
    boom = DB.GoError("Checksum mismatch")
    write, read = M.NewMemStore(), M.NewMemStore()
    w_model, r_model = dm.ModelStore(), dm.ModelStore()
    for store, model in ((read, r_model), (write, w_model)):
        tag = b"w" if store is write else b"r"
        for k in ((b"both", b"dead", b"mem-empty", b"bad") if store is write else (b"both", b"read-only", b"dead")):
            v = b"" if k == b"mem-empty" else tag + k
            store.Upsert(k, v)
            model.upsert(k, v)
    write.Tombstone(b"dead")
    w_model.tombstone(b"dead")
    view = DB.DBReadView(_Tables(tables, {b"bad": boom}), write, read)
    for k in (b"t", b"empty", b"nil", b"both", b"dead", b"mem-empty", b"read-only", b"absent"):
        v, e = view.GetBytes(k)
        assert (v, _err(e)) == dm.get_bytes(tables, w_model, r_model, k), k
        assert e is None or e is DB.ErrNotFound
    assert view.GetBytes(b"t") == (b"new", None) and view.GetBytes(b"mem-empty") == (b"", None)
    assert view.GetBytes(b"empty") == (None, DB.ErrNotFound) and view.GetBytes(b"nil") == (None, DB.ErrNotFound)
    assert view.GetBytes(b"bad") == (None, boom)  # the table's error, although the write store holds the key
    assert view.Get("both") == ("wboth", None) and view.Get("absent") == ("", DB.ErrNotFound)
    no_tables = DB.DBReadView(None, write)
    assert no_tables.GetBytes(b"t") == (None, DB.ErrNotFound) and no_tables.GetBytes(b"both") == (b"wboth", None)
    assert str(DB.ErrNotFound) == "ErrNotFound" and L.RIO_GET_MEM_VALUE == 4 and L.RIO_DB_MAX_MEMSTORES == 2


def test_new_calls_refuse_arguments_before_any_device_call():
    """RIO_ERR_ARG / RIO_ERR_UNSUPPORTED come back before the context, the reader or the device is touched: the
    calls are made with placeholder handles and device pointers on a machine that may have no GPU."""
    lib = L.lib()
    ctx, ptr = ctypes.c_void_p(8), ctypes.c_void_p(64)
    ops = L.OpsView(keys=64, key_off=64, values=64, val_off=64, flags=64, n=5, key_bytes=10, value_bytes=10)
    av = ctypes.addressof

    def build(c=ctx, o=ops, max_key_len=8, order=ptr, pfx=ptr, res=ptr):
        return lib.rio_mem_index_build(c, None if o is None else av(o), max_key_len, order, pfx, res, None)

    assert build(c=None) == L.RIO_ERR_ARG
    assert build(o=None) == L.RIO_ERR_ARG
    assert build(res=None) == L.RIO_ERR_ARG
    assert build(order=None) == L.RIO_ERR_ARG
    assert build(pfx=None) == L.RIO_ERR_ARG
    for field in ("keys", "key_off", "values", "val_off", "flags"):
        kw = {k: getattr(ops, k) for k, _ in L.OpsView._fields_}
        kw[field] = None
        assert build(o=L.OpsView(**kw)) == L.RIO_ERR_ARG, field
    assert build(max_key_len=L.RIO_FLUSH_MAX_KEY_LEN + 1) == L.RIO_ERR_UNSUPPORTED
    huge = {k: getattr(ops, k) for k, _ in L.OpsView._fields_}
    huge["n"] = (1 << 31) - 1
    assert build(o=L.OpsView(**huge)) == L.RIO_ERR_UNSUPPORTED

    good = L.MemIndex(ops=ops, order=64, pfx=64, result=64)
    one, two = (L.MemIndex * 1)(good), (L.MemIndex * 3)(good, good, good)

    def bad_indexes():
        yield None, 1
        yield one, 0
        yield two, 3
        yield (L.MemIndex * 1)(L.MemIndex(ops=ops, order=64, pfx=64, result=None)), 1
        yield (L.MemIndex * 1)(L.MemIndex(ops=ops, order=None, pfx=64, result=64)), 1
        yield (L.MemIndex * 2)(good, L.MemIndex(ops=ops, order=64, pfx=None, result=64)), 2

    def lookup(c=ctx, idx=one, k=1, keys=ptr, off=ptr, n=3, out=ptr):
        return lib.rio_mem_lookup(c, None if idx is None else av(idx), k, keys, off, n, 10, out, None)

    assert lookup(c=None) == L.RIO_ERR_ARG
    for idx, k in bad_indexes():
        assert lookup(idx=idx, k=k) == L.RIO_ERR_ARG
    assert lookup(keys=None) == L.RIO_ERR_ARG and lookup(off=None) == L.RIO_ERR_ARG and lookup(out=None) == L.RIO_ERR_ARG
    assert lookup(n=(1 << 31) - 1) == L.RIO_ERR_UNSUPPORTED
    assert lookup(n=0, keys=None, off=None, out=None) == L.RIO_OK  # no queries: nothing is touched

    h = ctypes.c_void_p()
    assert lib.rio_db_reader_create(None, None, 16, ctypes.byref(h)) == L.RIO_ERR_ARG
    assert lib.rio_db_reader_create(ctx, None, 16, None) == L.RIO_ERR_ARG
    assert lib.rio_db_reader_create(ctx, None, 0, ctypes.byref(h)) == L.RIO_ERR_ARG
    assert lib.rio_db_reader_create(ctx, None, (1 << 31) - 1, ctypes.byref(h)) == L.RIO_ERR_UNSUPPORTED
    assert not h.value
    lib.rio_db_reader_free(None)

    # a reader whose every field is zero: max_batch = 0, so n = 1 is n > max_batch, refused on the reader's own
    # fields before any device call (the bytes stand in for the handle on a machine without a GPU)
    blank = ctypes.create_string_buffer(512)
    rd = ctypes.c_void_p(ctypes.addressof(blank))

    def plan(r=rd, idx=one, k=1, tab=None, mem=ptr, n=1, status=ptr, val_off=ptr):
        return lib.rio_db_value_plan(r, None if idx is None else av(idx), k, tab, mem, n, 1, status, val_off, None)

    def copy(r=rd, idx=one, k=1, tab=None, mem=ptr, status=ptr, n=1, val_off=ptr, values=ptr):
        return lib.rio_db_value_copy(r, None if idx is None else av(idx), k, tab, mem, status, n, val_off, values, 10, None)

    for call in (plan, copy):
        assert call(r=None) == L.RIO_ERR_ARG
        for idx, k in bad_indexes():
            assert call(idx=idx, k=k) == L.RIO_ERR_ARG
        assert call(mem=None) == L.RIO_ERR_ARG and call(status=None) == L.RIO_ERR_ARG
        assert call(n=1) == L.RIO_ERR_ARG  # n > max_batch
    assert plan(val_off=None, n=0) == L.RIO_ERR_ARG
    assert copy(val_off=None) == L.RIO_ERR_ARG and copy(values=None) == L.RIO_ERR_ARG
