"""SuperSSTableReader on the host (no GPU): the stack model (tests/super_model.py) against the compaction model's
latest-wins merge, the C-ABI's argument checks of the stack calls, and the mirror's host-only parts."""
import ctypes
import random

import compact_model as cm
import super_model as sm

import sstables
from recordio import _lib as L


def _corpus(seed, n_tables, n_keys):
    rng = random.Random(seed)
    pool = [rng.randbytes(rng.randint(0, 12)) for _ in range(n_keys)] + [b"", b"a", b"a\0", b"prefix_8x", b"prefix_8y"]
    tables = []
    for _ in range(n_tables):
        t = {}
        for k in rng.sample(pool, rng.randint(0, len(pool))):
            t[k] = rng.choice([None, b"", rng.randbytes(rng.randint(1, 9))])
        tables.append(t)
    return pool, tables


def test_model_equals_the_latest_wins_merge():
    for seed in range(6):
        pool, tables = _corpus(seed, 1 + seed, 60)
        st = sm.Stack(tables)
        want = cm.merge_compact([sorted(t.items()) for t in tables], cm.reduce_latest_wins)
        assert st.scan() == want
        merged = dict(want)
        for k in pool:
            v = st.get(k)
            assert st.contains(k) == (v is not sm.NOT_FOUND)
            # the merge drops a key whose newest value is nil; Get returns that nil
            assert (v if v is not sm.NOT_FOUND and v is not None else None) == merged.get(k)
        lo, hi = sorted(pool)[len(pool) // 4], sorted(pool)[3 * len(pool) // 4]
        assert st.scan(lo) == [(k, v) for k, v in want if k >= lo]
        assert st.scan(lo, hi) == [(k, v) for k, v in want if lo <= k <= hi]
        assert st.scan(hi, lo) == []


def test_model_metadata_rule():
    metas = [(3, 10, 20, 30, 1, b"b", b"d"), (2, 1, 2, 3, 1, b"a", b"z"), (1, 1, 1, 2, 0, b"c", b"e")]
    # both keys end as the largest seen: the reference replaces MinKey when the running one is LOWER
    assert sm.metadata(metas) == (6, 12, 23, 35, 0, b"c", b"z")
    assert sm.metadata([]) == (0, 0, 0, 0, 0, b"", b"")


def test_every_stack_symbol_is_bound():
    names = ("rio_sst_stack_create", "rio_sst_stack_free", "rio_sst_stack_lookup", "rio_sst_stack_value_plan",
             "rio_sst_stack_value_copy", "rio_sst_stack_bounds", "rio_sst_keys_gather")
    lib = L.lib()
    assert all(n in L.EXPORTED and hasattr(lib, n) for n in names)
    assert (L.RIO_GET_VALUE, L.RIO_GET_NOT_FOUND, L.RIO_GET_NIL, L.RIO_GET_HOST) == (0, 1, 2, 3)


def test_stack_calls_refuse_arguments_before_any_device_call():
    """RIO_ERR_ARG comes back before the context, the stack or the device is touched: the calls are made with
    placeholder handles and device pointers on a machine that may have no GPU."""
    lib = L.lib()
    ctx, ptr = ctypes.c_void_p(8), ctypes.c_void_p(64)
    sst = L.SstView(index=64, key_off=64, key_len=64, data=64, data_off=64, flags=64, crc=64, n=5, index_bytes=10,
                    data_bytes=10)
    views, pfx = (L.SstView * 1)(sst), (ctypes.c_uint64 * 1)(64)
    h = ctypes.c_void_p()

    def create(c=ctx, v=views, p=pfx, f=None, T=1, max_batch=16, out=ctypes.byref(h)):
        av = lambda x: None if x is None else ctypes.addressof(x)  # noqa: E731
        return lib.rio_sst_stack_create(c, av(v), av(p), av(f), None, T, max_batch, out, None)

    assert create(c=None) == L.RIO_ERR_ARG
    assert create(v=None) == L.RIO_ERR_ARG
    assert create(p=None) == L.RIO_ERR_ARG
    assert create(out=None) == L.RIO_ERR_ARG
    assert create(T=0) == L.RIO_ERR_ARG
    assert create(T=L.RIO_MERGE_MAX_TABLES + 1) == L.RIO_ERR_ARG
    assert create(max_batch=0) == L.RIO_ERR_ARG
    assert create(p=(ctypes.c_uint64 * 1)(0)) == L.RIO_ERR_ARG  # a table with entries and no prefixes
    for bad in (dict(k=0), dict(k=L.RIO_BLOOM_MAX_K + 1), dict(m=1), dict(m=0), dict(hash_keys=None)):
        kw = dict(bits=64, hash_keys=64, m=9586, k=7)
        kw.update(bad)
        assert create(f=(L.BloomView * 1)(L.BloomView(**kw))) == L.RIO_ERR_ARG, bad
    assert not h.value
    lib.rio_sst_stack_free(None)
    # the stack calls: a NULL stack, then NULL arrays, before the stack is read
    st = ctypes.c_void_p(8)
    assert lib.rio_sst_stack_lookup(None, 0, ptr, ptr, 3, 10, ptr, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_stack_lookup(st, 2, ptr, ptr, 3, 10, ptr, None) == L.RIO_ERR_ARG
    for args in ((None, ptr, ptr), (ptr, None, ptr), (ptr, ptr, None)):
        assert lib.rio_sst_stack_lookup(st, 1, args[0], args[1], 3, 10, args[2], None) == L.RIO_ERR_ARG
    assert lib.rio_sst_stack_value_plan(None, ptr, 3, 0, ptr, ptr, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_stack_value_plan(st, None, 3, 0, ptr, ptr, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_stack_value_plan(st, ptr, 3, 0, None, ptr, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_stack_value_plan(st, ptr, 3, 0, ptr, None, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_stack_value_copy(None, ptr, 3, ptr, ptr, 10, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_stack_value_copy(st, None, 3, ptr, ptr, 10, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_stack_value_copy(st, ptr, 3, None, ptr, 10, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_stack_value_copy(st, ptr, 3, ptr, None, 10, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_stack_bounds(None, ptr, ptr, 1, 10, 0, ptr, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_stack_bounds(st, ptr, ptr, 1, 10, 2, ptr, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_stack_bounds(st, None, ptr, 1, 10, 0, ptr, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_stack_bounds(st, ptr, None, 1, 10, 1, ptr, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_stack_bounds(st, ptr, ptr, 1, 10, 1, None, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_stack_bounds(st, ptr, ptr, 0, 10, 1, None, None) == L.RIO_OK  # no keys: nothing is touched
    assert lib.rio_sst_keys_gather(None, ptr, 3, ptr, 10, ptr, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_keys_gather(ctx, None, 3, ptr, 10, ptr, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_keys_gather(ctx, ptr, 3, None, 10, ptr, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_keys_gather(ctx, ptr, 3, ptr, 10, None, None) == L.RIO_ERR_ARG


class _Reader:
    """What SuperSSTableReader's host loops need of a reader."""

    def __init__(self, table, path, meta, fail=None):
        self.table, self.path, self.meta, self.fail, self.closed = table, path, meta, fail, False

    def Get(self, key):  # noqa: N802
        if self.fail is not None:
            return None, self.fail
        return (self.table[key], None) if key in self.table else (None, sstables.NotFound)

    def Contains(self, key):  # noqa: N802
        return (False, self.fail) if self.fail is not None else (key in self.table, None)

    def MetaData(self):  # noqa: N802
        return self.meta

    def BasePath(self):  # noqa: N802
        return self.path

    def Close(self):  # noqa: N802
        self.closed = True
        return self.fail


def test_host_loops_metadata_basepath_close():
    _, tables = _corpus(11, 4, 40)
    metas = [sstables.proto.MetaData(numRecords=len(t), minKey=min(t, default=b""), maxKey=max(t, default=b""),
                                     dataBytes=7 * i, indexBytes=3 * i, totalBytes=10 * i, version=1)
             for i, t in enumerate(tables)]
    readers = [_Reader(t, f"/p/{i}", m) for i, (t, m) in enumerate(zip(tables, metas))]
    sr = sstables.NewSuperSSTableReader(readers)
    st = sm.Stack(tables)
    for k in sorted(set().union(*tables)) + [b"absent", b"\xff\xff"]:
        want = st.get(k)
        assert sr.Get(k) == ((None, sstables.NotFound) if want is sm.NOT_FOUND else (want, None))
        assert sr.Contains(k) == (st.contains(k), None)
    m = sr.MetaData()
    want = sm.metadata([(x.numRecords, x.dataBytes, x.indexBytes, x.totalBytes, x.version, x.minKey, x.maxKey)
                        for x in metas])
    assert (m.numRecords, m.dataBytes, m.indexBytes, m.totalBytes, m.version, m.minKey, m.maxKey) == want
    # reproduced, not fixed: MinKey is the LARGEST of the readers' minimum keys
    assert (m.minKey, m.maxKey) == (max(x.minKey for x in metas), max(x.maxKey for x in metas))
    assert sr.BasePath() == "/p/0,/p/1,/p/2,/p/3"
    # another comparator orders MetaData's keys (the reference calls comp.Compare there); BytesComparator is the default
    rev = sstables.NewSuperSSTableReader(readers, comp=lambda a, b: -sstables.BytesComparator(a, b)).MetaData()
    assert (rev.minKey, rev.maxKey) == (b"", b"")  # nothing compares above the empty running key
    same = sstables.NewSuperSSTableReader(readers, comp=sstables.BytesComparator).MetaData()
    assert (same.minKey, same.maxKey) == (m.minKey, m.maxKey)
    # readers that are not device tables: the batched calls and the scans hand back UnsupportedError
    assert all(isinstance(e, sstables.UnsupportedError) for _, e in sr.GetBatch([b"a", b"b"]))
    assert all(isinstance(e, sstables.UnsupportedError) for _, e in sr.ContainsBatch([b"a"]))
    for it, err in (sr.Scan(), sr.ScanStartingAt(b"a"), sr.ScanRange(b"a", b"b")):
        assert it is None and isinstance(err, sstables.UnsupportedError)
    assert sr.Close() is None and all(r.closed for r in readers)
    assert sr.Close() is None  # again: harmless


def test_an_error_of_a_newer_reader_is_returned():
    from recordio.errors import GoError

    boom = GoError("boom")
    old, new = _Reader({b"k": b"old"}, "/o", None), _Reader({}, "/n", None, fail=boom)
    sr = sstables.NewSuperSSTableReader([old, new])
    assert sr.Get(b"k") == (None, boom) and sr.Contains(b"k") == (False, boom)
    assert sstables.NewSuperSSTableReader([new, old]).Get(b"k") == (b"old", None)  # the newer table answers first
    assert str(sr.Close()) == "boom"
