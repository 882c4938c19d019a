"""Batched GetBytes on the device (GPU): rio_mem_index_build / rio_mem_lookup (csrc/rio_memidx.hip), rio_db_value_plan /
rio_db_value_copy (csrc/rio_db.hip) and the mirror (memstore.DeviceMemIndex, MemStore.GetBatch, simpledb.DBReadView).
Every case compares GetBatch, the loop of GetBytes and the model (tests/db_model.py: db.go:197-242 over
rw_memstore.go), and GetBatchOnDevice's source words, statuses, offsets and bytes with the model."""
import ctypes
import os
import random
import struct

import numpy as np
import pytest
import torch

import db_model as dm
import memstore as M
import simpledb as DB
import sstables as S
from conftest import GOLDEN
from recordio import _lib as L
from sstables.writer import write_sstable

pytestmark = pytest.mark.gpu

_NONE = 0xFFFFFFFFFFFFFFFF
BITS = L.RIO_MERGE_ENTRY_BITS
MAXK = L.RIO_FLUSH_MAX_KEY_LEN
P8 = b"prefix_8"


def be(i):
    return struct.pack(">I", i)


def val(n, seed):
    return bytes((seed * 31 + 7 * j) & 0xFF for j in range(n))


def stores(ops):
    """A MemStore and its model after `ops` = [(key, value or None for a tombstone)]."""
    ms, model = M.NewMemStore(), dm.ModelStore()
    apply(ms, model, ops)
    return ms, model


def apply(ms, model, ops):
    for k, v in ops:
        if v is None:
            assert ms.Tombstone(k) is None
            model.tombstone(k)
        else:
            assert ms.Upsert(k, v) is None
            model.upsert(k, v)


def open_stack(tmp_path, tables, opts=(), name="t", **kw):
    readers = []
    for i, t in enumerate(tables):
        base = str(tmp_path / f"{name}{i}")
        write_sstable(base, sorted(t.items()))
        r, err = S.NewSSTableReader(S.ReadBasePath(base), *opts)
        assert err is None, err
        readers.append(r)
    return S.NewSuperSSTableReader(readers, **kw)


def arena(queries):
    """The queries back to back with NO byte after the last one."""
    raw = b"".join(queries)
    d_keys = torch.from_numpy(np.frombuffer(raw or b"\0", dtype=np.uint8).copy()).cuda()
    d_off = torch.from_numpy(np.cumsum([0] + [len(q) for q in queries]).astype(np.int64)).cuda()
    return d_keys[:len(raw)] if raw else d_keys[:0], d_off, len(raw)


def same(batch, loop):
    assert len(batch) == len(loop)
    for i, ((bv, berr), (lv, lerr)) in enumerate(zip(batch, loop)):
        assert bv == lv and type(bv) is type(lv), i
        assert (berr is None) == (lerr is None) and str(berr) == str(lerr), i
        assert (berr is DB.ErrNotFound) == (lerr is DB.ErrNotFound), i


def want_device(tables, w, r, queries):
    """(mem words, table words, statuses, offsets, bytes) the model expects of GetBatchOnDevice."""
    mem, tab, status, vals = [], [], [], []
    models = [s for s in (r, w) if s is not None]
    memo = {}
    for q in queries:
        if q not in memo:
            m, t = dm.mem_source(w, r, q), dm.table_source(tables, q)
            if m is not None:
                v = models[m[0]].ops[m[1]][1]
                st = L.RIO_GET_NOT_FOUND if v is None else L.RIO_GET_MEM_VALUE
            else:
                v = (tables[t[0]][q] if t is not None else None) or None
                st = L.RIO_GET_NOT_FOUND if v is None else L.RIO_GET_VALUE
            memo[q] = (_NONE if m is None else (m[0] << BITS) | m[1], _NONE if t is None else (t[0] << BITS) | t[1], st, v or b"")
        for out, x in zip((mem, tab, status, vals), memo[q]):
            out.append(x)
    off = np.cumsum([0] + [len(v) for v in vals]).tolist()
    return mem, tab, status, off, b"".join(vals)


def on_device(view, queries):
    d_keys, d_off, _ = arena(queries)
    mem, tab, status, val_off, values = view.GetBatchOnDevice(d_keys, d_off, len(queries))
    torch.cuda.synchronize()
    words = lambda t: None if t is None else [x & _NONE for x in t.cpu().tolist()]  # noqa: E731
    return words(mem), words(tab), status.cpu().tolist(), val_off.cpu().tolist(), bytes(values.cpu().numpy())


def check(view, tables, w, r, queries):
    """GetBatch == the loop of GetBytes == the model; the device tensors are the model's."""
    memo = {}
    for q in set(queries):
        memo[q] = view.GetBytes(q)
        v, e = memo[q]
        assert (v, None if e is None else str(e)) == dm.get_bytes(tables, w, r, q), q
        assert e is None or e is DB.ErrNotFound
    gets = [memo[q] for q in queries]  # GetBytes is a pure function of the key: the loop, without repeating keys
    same(view.GetBatch(queries), gets)
    mem, tab, status, off, raw = on_device(view, queries)
    w_mem, w_tab, w_status, w_off, w_raw = want_device(tables, w, r, queries)
    assert mem == w_mem and status == w_status and off == w_off and raw == w_raw
    assert tab == (w_tab if view.tables is not None else None)
    return gets


def check_index(ms, model):
    """order and pfx read back: the model's keys in sorted() order, each with its latest op and its prefix."""
    idx = ms._index()
    torch.cuda.synchronize()
    words = idx.result_words()
    keys = sorted(model.latest)
    assert words[L.RIO_MERGE_R_N_OUT] == idx.n_keys() == len(keys) and words[L.RIO_MERGE_R_UNSORTED] == _NONE
    order = [x & _NONE for x in idx.order[:len(keys)].cpu().tolist()]
    pfx = [x & _NONE for x in idx.pfx[:len(keys)].cpu().tolist()]
    assert order == [model.source(k) for k in keys]
    assert pfx == [int.from_bytes(k[:8].ljust(8, b"\0"), "big") for k in keys]


# ---- index sizes ---------------------------------------------------------------------------------------------------

LOGS = {
    "empty": [],
    "one key": [(b"k1", b"v1")],
    "two keys": [(b"k2", b"v2"), (b"k1", b"v1")],
    "three keys": [(b"k2", b"v2"), (b"k3", b""), (b"k1", b"v1")],
    "put delete put": [(b"k", b"first"), (b"k", None), (b"k", b"third")],
    "put put delete": [(b"k", b"first"), (b"k", b"second"), (b"k", None)],
    "tombstones only": [(b"k3", None), (b"k1", None), (b"k2", None), (b"k1", None)],
}


@pytest.mark.parametrize("name", list(LOGS))
def test_index_sizes(name):
    ms, model = stores(LOGS[name])
    check_index(ms, model)
    view = DB.DBReadView(None, ms)
    queries = [b"k", b"k0", b"k1", b"k2", b"k3", b"k4", b"", b"k1\0", b"zz"]
    check(view, None, model, None, queries)
    same(ms.GetBatch(queries), [ms.Get(q) for q in queries])
    for (_, be_), (_, le) in zip(ms.GetBatch(queries), [ms.Get(q) for q in queries]):
        assert be_ is le  # KeyNotFound / KeyTombstoned themselves
    assert ms.ContainsBatch(queries) == [ms.Contains(q) for q in queries] == [model.contains(q) for q in queries]
    view.Close()


# ---- key shapes and query places -----------------------------------------------------------------------------------

LONG = b"L" * (MAXK - 1)
FORMS = [b"a", b"a\0", b"a\0\0", b"ab", b"abc\0\0\0\0", b"ab\0\0\0\0\0\0", b"ab\0\0\0\0\0\0\0", P8, P8 + b"\0", P8 + b"x",
         P8 + b"y", P8 + b"xx", P8 + b"xxlong-tail-A", P8 + b"xxlong-tail-B", b"prefix_", b"\xfe\xff", LONG + b"x"]


def test_key_shapes_and_query_places():
    assert len(LONG + b"x") == MAXK
    write, w = stores([(k, b"w:" + k[:20]) for k in FORMS[::-1]] + [(b"a\0", None), (P8 + b"x", b"again")])
    read, r = stores([(b"", b"the empty key"), (b"a", b"read-a"), (b"zz-read", b"r")])
    check_index(write, w)
    check_index(read, r)
    view = DB.DBReadView(None, write, read)
    queries = list(FORMS) + [
        b"",                                   # below the write store's first key (the read store holds it)
        b"\x00", b"\xff\xff\xff",              # below every non-empty key, above the last
        b"aa", P8 + b"w", b"b",                # between two keys
        P8 + b"z", P8 + b"xy", P8 + b"\0\0",   # absent with a present key's prefix
        b"prefix", P8 + b"xxlong-tail-", P8 + b"xxlong-tail-AA", P8 + b"xxlong-tail-C",  # proper prefixes, extensions
        b"a\0\0\0", b"ab\0", LONG, LONG + b"xy", LONG + b"y", b"zz-read",
        P8 + b"xxlong-tail-B",                 # the last query ends at the arena's last byte
    ]
    gets = check(view, None, w, r, queries)
    assert gets[queries.index(b"")] == (b"the empty key", None) and gets[queries.index(LONG + b"x")][1] is None
    assert gets[queries.index(b"a\0")] == (None, DB.ErrNotFound) and gets[queries.index(b"a")] == (b"w:a", None)
    view.Close()


def test_a_key_longer_than_the_bound_is_refused():
    ms, model = stores([(b"fine", b"v"), (b"K" * (MAXK + 1), b"too long")])
    got = ms.GetBatch([b"fine", b"absent"])
    assert all(v is None and isinstance(e, S.UnsupportedError) and f"{MAXK + 1} bytes" in str(e) for v, e in got)
    words = ms._index().result_words()
    assert words[L.RIO_MERGE_R_N_OUT] == 0 and words[L.RIO_MERGE_R_UNSORTED] == 1  # the device refuses the log too
    with pytest.raises(S.UnsupportedError):
        ms.ContainsBatch([b"fine"])
    view = DB.DBReadView(None, ms)
    assert all(isinstance(e, S.UnsupportedError) for _, e in view.GetBatch([b"fine", b"x"]))
    d_keys, d_off, _ = arena([b"fine"])
    with pytest.raises(S.UnsupportedError):
        view.GetBatchOnDevice(d_keys, d_off, 1)


# ---- precedence: one case per rule of rio_db_value_plan ------------------------------------------------------------

K = b"the-key"
PRECEDENCE = {
    # name: (tables or None, write ops, read ops or None, (value, found))
    "rule 3: a write-store tombstone over a read-store value over a table value":
        ([{K: b"table"}], [(K, b"w"), (K, None)], [(K, b"read")], None),
    "rule 2: a write-store miss with the read-store value": ([{K: b"table"}], [(b"other", b"w")], [(K, b"read")], b"read"),
    "rule 3: a read-store tombstone over a table value": ([{K: b"table"}], [(b"other", b"w")], [(K, None)], None),
    "rule 4: both stores miss and the table has the value": ([{K: b"old"}, {K: b"table"}], [(b"o", b"w")], [(b"p", b"r")], b"table"),
    "rule 2: a memstore empty value over a table value": ([{K: b"table"}], [(K, b"")], [(K, b"read")], b""),
    "rule 5: the table value is empty": ([{K: b"older"}, {K: b""}], [(b"o", b"w")], [(b"p", b"r")], None),
    "rule 5: the table value is nil": ([{K: b"older"}, {K: None}], [(b"o", b"w")], None, None),
    "rule 5: no store and no table holds the key": ([{b"q": b"x"}], [(b"o", b"w")], [(b"p", b"r")], None),
    "rule 2: tables=None": (None, [(K, b"mem")], [(K, b"read")], b"mem"),
    "rule 2: one store only": ([{K: b"table"}], [(K, b"mem")], None, b"mem"),
    "rule 4: one store only, which misses": ([{K: b"table"}], [(b"o", b"w")], None, b"table"),
}


@pytest.mark.parametrize("name", list(PRECEDENCE))
def test_precedence(tmp_path, name):
    tables, w_ops, r_ops, want = PRECEDENCE[name]
    write, w = stores(w_ops)
    read, r = stores(r_ops) if r_ops is not None else (None, None)
    sr = open_stack(tmp_path, tables) if tables is not None else None
    view = DB.DBReadView(sr, write, read)
    queries = [K, b"other", b"o", b"p", b"q", b"absent", K + b"\0", K[:-1]]
    gets = check(view, tables, w, r, queries)
    assert gets[0] == ((None, DB.ErrNotFound) if want is None else (want, None))
    view.Close()
    if sr is not None:
        sr._free_stack()


def test_a_table_read_error_wins_over_the_memstore(tmp_path):
    """rule 1: the reference's CRCHashesMismatch table (its fourth value has a flipped byte) read with hash checks
    on reads, while the write store holds the same key: the table's error comes back (db.go:212-218)."""
    older = {be(i): b"good%d" % i for i in range(0, 10)}
    write_sstable(str(tmp_path / "older"), sorted(older.items()))
    r0, err = S.NewSSTableReader(S.ReadBasePath(str(tmp_path / "older")), S.EnableHashCheckOnReads())
    assert err is None, err
    r1, err = S.NewSSTableReader(S.ReadBasePath(os.path.join(GOLDEN, "sstables", "SimpleWriteHappyPathSSTableWithCRCHashesMismatch")),
                                 S.SkipHashCheckOnLoad(), S.EnableHashCheckOnReads())
    assert err is None, err
    sr = S.NewSuperSSTableReader([r0, r1])
    write, _ = stores([(be(4), b"memstore holds it"), (be(5), b"mem5"), (be(6), None)])
    view = DB.DBReadView(sr, write)
    queries = [be(i) for i in range(0, 12)]
    gets = [view.GetBytes(q) for q in queries]
    same(view.GetBatch(queries), gets)
    assert gets[4][0] is None and "Checksum mismatch: expected 688fffff90000000, got 738fffff90000000" in str(gets[4][1])
    assert gets[5] == (b"mem5", None) and gets[6] == (None, DB.ErrNotFound) and gets[0] == (b"good0", None)
    mem, tab, status, off, raw = on_device(view, queries)
    assert status[4] == L.RIO_GET_HOST and mem[4] == 0 and tab[4] == (1 << BITS) | 3 and off[4] == off[5]
    assert status[5] == L.RIO_GET_MEM_VALUE and status[6] == L.RIO_GET_NOT_FOUND and status[0] == L.RIO_GET_VALUE
    view.Close()
    sr._free_stack()


# ---- value lengths -------------------------------------------------------------------------------------------------

def test_value_lengths_round_the_long_value_split(tmp_path):
    lens = [0, 1, 1023, 1024, 1025]
    write, w = stores([(b"m%d" % n, val(n, n)) for n in lens] + [(b"big", val(70000, 3))])
    tables = [{b"t%d" % i: val(i + 1, i) for i in range(6)} | {b"big": b"hidden", b"tlong": val(1500, 9)}]
    sr = open_stack(tmp_path, tables)
    view = DB.DBReadView(sr, write)
    queries = [b"t0", b"m1024", b"big", b"t1", b"m0", b"m1023", b"tlong", b"m1", b"t5", b"m1025", b"none", b"t2"]
    gets = check(view, tables, w, None, queries)
    assert gets[2] == (val(70000, 3), None) and gets[4] == (b"", None)
    view.Close()
    sr._free_stack()


# ---- launch shapes -------------------------------------------------------------------------------------------------

def test_more_queries_than_one_grid_and_pieces_of_max_batch(tmp_path):
    tables = [{be(1): b"t1", be(2): b"t2", be(3): b"t3"}]
    ops = [(be(2), b"m2"), (be(3), None), (be(9), b"m9")]
    write, w = stores(ops)
    sr = open_stack(tmp_path, tables)
    view = DB.DBReadView(sr, write)
    n = 2048 * 256 + 1  # the grid-stride loops of 2048 blocks x 256 lanes go round again
    queries = [be(i % 11) for i in range(n)]
    check(view, tables, w, None, queries)
    view.Close()
    small = DB.DBReadView(sr, write, max_batch=5)
    twelve = [be(i) for i in (9, 1, 2, 3, 4, 0, 9, 9, 3, 2, 1, 7)]
    same(small.GetBatch(twelve), [small.GetBytes(q) for q in twelve])
    assert [v for v, _ in small.GetBatch(twelve)] == [dm.get_bytes(tables, w, None, q)[0] for q in twelve]
    # n > max_batch is refused by the reader itself
    d_keys, d_off, _ = arena(twelve)
    with pytest.raises(DB.GoError):
        small.GetBatchOnDevice(d_keys, d_off, 12)
    small.Close()
    sr._free_stack()


# ---- rebuild -------------------------------------------------------------------------------------------------------

FIRST = [(b"k%02d" % i, b"v%d" % i) for i in range(20)]
MORE = [(b"k03", b"overwritten"), (b"k05", None), (b"k20", b"added"), (b"a-new-first", b"x"), (b"k07", b""), (b"k05", b"back")]


def test_a_memstore_that_grows_is_indexed_again():
    ms, model = stores(FIRST)
    view = DB.DBReadView(None, ms)
    queries = [k for k, _ in FIRST] + [b"k20", b"a-new-first", b"absent"]
    check(view, None, model, None, queries)
    first_index = ms._index()
    apply(ms, model, MORE)
    check(view, None, model, None, queries)
    assert ms._index() is first_index and first_index.ops.n == len(FIRST) + len(MORE)
    check_index(ms, model)
    view.Close()


def _batch(ops):
    b = DB.WriteBatch()
    for k, v in ops:
        assert (b.DeleteBytes(k) if v is None else b.PutBytes(k, v)) is None
    return b


def _appender(path):
    import recordio as R
    import wal as W

    os.makedirs(path)
    opts, err = W.NewWriteAheadLogOptions(W.BasePath(path), W.MaximumWalFileSizeBytes(1 << 20),
                                          W.WriterFactory(lambda p: R.NewFileWriter(p, L.COMP_SNAPPY)))
    assert err is None, err
    a, err = W.NewAppender(opts)
    assert err is None, err
    return a


def test_a_log_append_batch_returned_is_read_without_the_host(tmp_path):
    a = _appender(str(tmp_path / "wal"))
    model = dm.ModelStore()
    queries = [k for k, _ in FIRST] + [b"k20", b"a-new-first", b"absent"]
    idx = None
    for ops in (FIRST, FIRST + MORE):  # the second batch is the longer log: the index is rebuilt over it
        dev_ops, err = DB.append_batch(a, _batch(ops))
        assert err is None, err
        model = dm.ModelStore()
        for k, v in ops:
            model.tombstone(k) if v is None else model.upsert(k, v)
        idx = M.DeviceMemIndex(dev_ops) if idx is None else idx.rebuild(dev_ops)
        view = DB.DBReadView(None, idx)
        check(view, None, model, None, queries)
        same([idx.Get(q) for q in queries], [(v, None if e is None else (M.KeyNotFound if e == dm.KEY_NOT_FOUND else M.KeyTombstoned))
                                            for v, e in (model.get(q) for q in queries)])
        view.Close()
    assert a.Close() is None


def _recovered_ops(base_path):
    """The directory's WAL files decoded on the device and turned into an op log (simpledb.recover_wal's first half)."""
    from recordio.device import DeviceDecoder, to_device_file
    from wal import _wal_files

    paths = _wal_files(base_path)
    files = [to_device_file(open(p, "rb").read(), 0) for p in paths]
    decoded = DeviceDecoder(0).decode_batch(files)
    segs = []
    for path, (buf, info) in zip(paths, decoded):
        n, err = DB._cut(path, buf, info)
        assert err is None, err
        segs.append(L.WalSegment(out=buf.out.data_ptr(), out_off=buf.out_off.data_ptr(), flags=buf.flags.data_ptr(), n=n,
                                 out_bytes=info["total_out_bytes"]))
    r, t = DB.wal_ops_on_device(L.default_ctx(0), 0, (L.WalSegment * len(segs))(*segs))
    assert r[L.RIO_WAL_R_FIRST_BAD] == _NONE
    ops = M.DeviceOps(0, t["keys"], t["key_off"], t["values"], t["val_off"], t["flags"], r[L.RIO_WAL_R_N_OPS],
                      r[L.RIO_WAL_R_KEY_BYTES], r[L.RIO_WAL_R_VALUE_BYTES], r[L.RIO_WAL_R_MAX_KEY_LEN])
    return ops, (decoded, files)


def test_a_recovered_log_is_read_without_the_host(tmp_path):
    wal_dir = str(tmp_path / "wal")
    a = _appender(wal_dir)
    _, err = DB.append_batch(a, _batch(FIRST))
    assert err is None, err
    more = [(k, v) for k, v in MORE if v != b""]  # an empty value does not survive the WAL: the replay refuses it as nil
    _, err = DB.append_batch(a, _batch(more))
    assert err is None and a.Close() is None
    ops, keep = _recovered_ops(wal_dir)
    assert ops.n == len(FIRST) + len(more)
    model = dm.ModelStore()
    for k, v in FIRST + more:
        model.tombstone(k) if v is None else model.upsert(k, v)
    view = DB.DBReadView(None, M.DeviceMemIndex(ops))
    check(view, None, model, None, [k for k, _ in FIRST] + [b"k20", b"a-new-first", b"absent"])
    view.Close()
    del keep


# ---- graph capture -------------------------------------------------------------------------------------------------

def test_lookups_and_plan_replay_from_one_graph_after_a_rebuild_in_place(tmp_path):
    """rio_sst_stack_lookup, rio_mem_lookup and rio_db_value_plan captured as one linear chain; the index is then
    rebuilt over a longer log into the same buffers and the replay answers from it: n_keys is read from device
    memory. The captured index names the buffers' capacity as ops.n; the builds name the log's length."""
    tables = [{be(i): b"table-%d" % i for i in range(0, 40)}]
    sr = open_stack(tmp_path, tables)
    short = [(be(i), b"mem-%d" % i) for i in range(30, 50, 3)]
    longer = short + [(be(33), None), (be(1), b"new"), (be(60), b""), (be(36), b"again")]
    cap_n, cap_k, cap_v = 32, 256, 512
    d = dict(keys=torch.zeros(cap_k + L.RIO_DEVICE_PAD, dtype=torch.uint8, device="cuda"),
             values=torch.zeros(cap_v + L.RIO_DEVICE_PAD, dtype=torch.uint8, device="cuda"),
             key_off=torch.zeros(cap_n + 1, dtype=torch.int64, device="cuda"),
             val_off=torch.zeros(cap_n + 1, dtype=torch.int64, device="cuda"),
             flags=torch.zeros(cap_n, dtype=torch.uint8, device="cuda"))
    order, pfx = (torch.zeros(cap_n, dtype=torch.int64, device="cuda") for _ in range(2))
    result = torch.zeros(L.RIO_MERGE_RESULT_WORDS, dtype=torch.int64, device="cuda")
    lib, ctx = L.lib(), L.default_ctx(0)

    def view_of(n, kb, vb):
        return L.OpsView(keys=d["keys"].data_ptr(), key_off=d["key_off"].data_ptr(), values=d["values"].data_ptr(),
                         val_off=d["val_off"].data_ptr(), flags=d["flags"].data_ptr(), n=n, key_bytes=kb, value_bytes=vb)

    def build(ops, st):
        """The log written into the fixed buffers (offsets past it repeat its end), then the index over it."""
        keys, vals = b"".join(k for k, _ in ops), b"".join(v or b"" for _, v in ops)
        ko = np.cumsum([0] + [len(k) for k, _ in ops]).tolist()
        vo = np.cumsum([0] + [len(v or b"") for _, v in ops]).tolist()
        fill = lambda o: torch.tensor(o + [o[-1]] * (cap_n + 1 - len(o)), dtype=torch.int64)  # noqa: E731
        d["keys"][:len(keys)].copy_(torch.from_numpy(np.frombuffer(keys, dtype=np.uint8).copy()))
        d["values"][:len(vals)].copy_(torch.from_numpy(np.frombuffer(vals, dtype=np.uint8).copy()))
        d["key_off"].copy_(fill(ko))
        d["val_off"].copy_(fill(vo))
        d["flags"][:len(ops)].copy_(torch.tensor([L.RIO_FLAG_NIL if v is None else 0 for _, v in ops], dtype=torch.uint8))
        ov = view_of(len(ops), len(keys), len(vals))
        assert lib.rio_mem_index_build(ctx, ctypes.addressof(ov), 4, order.data_ptr(), pfx.data_ptr(), result.data_ptr(), st) == 0

    n = 24
    queries = [be(i) for i in list(range(28, 50)) + [1, 60]]
    d_keys, d_off, nbytes = arena(queries)
    tab, mem = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    val_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    sr.GetBatch(queries[:2])  # the stack exists before the capture: nothing is created inside it
    reader = ctypes.c_void_p()
    assert lib.rio_db_reader_create(ctx, sr._stack, 64, ctypes.byref(reader)) == 0
    captured = (L.MemIndex * 1)(L.MemIndex(ops=view_of(cap_n, cap_k, cap_v), order=order.data_ptr(), pfx=pfx.data_ptr(),
                                           result=result.data_ptr()))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        build(short, ctypes.c_void_p(stream.cuda_stream))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.rio_sst_stack_lookup(sr._stack, 0, d_keys.data_ptr(), d_off.data_ptr(), n, nbytes, tab.data_ptr(), st) == 0
        assert lib.rio_mem_lookup(ctx, ctypes.addressof(captured), 1, d_keys.data_ptr(), d_off.data_ptr(), n, nbytes,
                                  mem.data_ptr(), st) == 0
        assert lib.rio_db_value_plan(reader, ctypes.addressof(captured), 1, tab.data_ptr(), mem.data_ptr(), n, 1,
                                     status.data_ptr(), val_off.data_ptr(), st) == 0
    answers = []
    for ops in (short, longer):
        with torch.cuda.stream(stream):
            build(ops, ctypes.c_void_p(stream.cuda_stream))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        w = dm.ModelStore()
        for k, v in ops:
            w.tombstone(k) if v is None else w.upsert(k, v)
        w_mem, w_tab, w_status, w_off, _ = want_device(tables, w, None, queries)
        assert [x & _NONE for x in mem.cpu().tolist()] == w_mem and [x & _NONE for x in tab.cpu().tolist()] == w_tab
        assert status.cpu().tolist() == w_status and val_off.cpu().tolist() == w_off
        answers.append(w_status)
    assert answers[0] != answers[1]  # the replay saw the rebuilt index
    lib.rio_db_reader_free(reader)
    sr._free_stack()


# ---- seeded sweep --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [11, 12, 13])
def test_seeded_sweep(tmp_path, seed):
    rng = random.Random(seed)
    universe = [b"key-%04d" % i + (b"-tail" * (i % 3)) for i in range(450)]
    present = universe[:300]
    tables = []
    for t in range(3):
        tables.append({k: (None if rng.randrange(10) == 0 else b"" if rng.randrange(12) == 0 else val(rng.randrange(1, 60), t))
                       for k in rng.sample(present, 200)})
    (read, r), (write, w) = stores([]), stores([])
    for i in range(2000):
        ms, model = (read, r) if i < 1000 else (write, w)
        k = rng.choice(present)
        v = None if rng.randrange(4) == 0 else val(rng.choice([0, 1, 7, 33, 200]), i)
        apply(ms, model, [(k, v)])
    sr = open_stack(tmp_path, tables)
    view = DB.DBReadView(sr, write, read, max_batch=400)
    absent = universe[300:] + [k + b"\0" for k in present[:100]] + [k[:-1] for k in present[:100]]
    queries = [rng.choice(absent) if i % 3 == 0 else rng.choice(present) for i in range(1000)]
    same(view.GetBatch(queries), [view.GetBytes(q) for q in queries])
    for a in range(0, 1000, 400):  # GetBatchOnDevice takes up to max_batch queries
        check(view, tables, w, r, queries[a:a + 400])
    view.Close()
    sr._free_stack()


# ---- clamping ------------------------------------------------------------------------------------------------------

def test_hostile_order_words_and_counts_stay_in_range():
    """A d_order word beyond n and an n_keys word above n, handed straight to rio_mem_lookup: every word that comes
    back is ~0 or names an op of the log, and the call returns."""
    ms, model = stores([(b"k%d" % i, b"v%d" % i) for i in range(8)])
    idx = ms._index()
    torch.cuda.synchronize()
    n = idx.ops.n
    queries = [b"k%d" % i for i in range(10)] + [b"", b"zz"]
    d_keys, d_off, nbytes = arena(queries)
    lib, ctx = L.lib(), L.default_ctx(0)
    out = torch.zeros(len(queries), dtype=torch.int64, device="cuda")

    def lookup(order, result):
        view = idx.view
        view.order, view.result = order.data_ptr(), result.data_ptr()
        arr = (L.MemIndex * 1)(view)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.rio_mem_lookup(ctx, ctypes.addressof(arr), 1, d_keys.data_ptr(), d_off.data_ptr(), len(queries), nbytes,
                                  out.data_ptr(), st) == 0
        torch.cuda.synchronize()
        return [x & _NONE for x in out.cpu().tolist()]

    honest = lookup(idx.order, idx.result)
    assert honest == [i if i < 8 else _NONE for i in range(10)] + [_NONE, _NONE]
    order = idx.order.clone()
    order[3] = n + 1000  # position 3 of the order (key k3) names an op that does not exist: read as op 0
    got = lookup(order, idx.result)
    assert all(w == _NONE or w < n for w in got) and got[:3] == honest[:3] and got[4:8] == honest[4:8]
    assert got[3] == 0  # wrong, in range: the probe's prefix stands for a short key's bytes, the op's lengths agree
    result = idx.result.clone()
    result[L.RIO_MERGE_R_N_OUT] = n + 5000  # clamped to n = the buffers' length
    got = lookup(idx.order, result)
    assert got == honest
