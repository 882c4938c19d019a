"""The memstore that grows on the device (GPU): rio_ops_append and rio_mem_index_extend (csrc/rio_memidx.hip) and the
mirror over them (memstore.DeviceOpLog, DeviceMemIndex.extend, DeviceMemStore, MemStore._index).

The yardstick of every index comparison is rio_mem_index_build over the same final log into separate buffers: equal
means order[:n_keys], pfx[:n_keys] and all RIO_MERGE_RESULT_WORDS result words. Where it is cheap the model's
answer (a dict of latest ops and sorted()) is compared too. The helpers are tests/test_gpu_db_get.py's, copied."""
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
from recordio import _lib as L
from sstables.writer import write_sstable

pytestmark = pytest.mark.gpu

_NONE = 0xFFFFFFFFFFFFFFFF
BITS = L.RIO_MERGE_ENTRY_BITS
MAXK = L.RIO_FLUSH_MAX_KEY_LEN
WORDS = L.RIO_MERGE_RESULT_WORDS
P8 = b"prefix_8"


# ---- helpers copied from tests/test_gpu_db_get.py -----------------------------------------------------------------

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
    gets = [memo[q] for q in queries]
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


# ---- a log, its prefixes and their indexes ------------------------------------------------------------------------

class Log:
    """`ops` = [(key, value or None)] as one op log in device memory, and views over its first k ops."""

    def __init__(self, ops):
        self.ops = ops
        self.ko = np.cumsum([0] + [len(k) for k, _ in ops]).tolist()
        self.vo = np.cumsum([0] + [len(v or b"") for _, v in ops]).tolist()
        keys, values = bytearray(b"".join(k for k, _ in ops)), bytearray(b"".join(v or b"" for _, v in ops))
        flags = bytearray(L.RIO_FLAG_NIL if v is None else 0 for _, v in ops)
        self.dev = M.upload_ops(0, keys, self.ko, values, self.vo, flags, self.bound(0, len(ops)))

    def bound(self, a, b):
        """The longest key of ops [a, b)."""
        return max([len(k) for k, _ in self.ops[a:b]] or [0])

    def view(self, k):
        v = self.dev.view
        return L.OpsView(keys=v.keys, key_off=v.key_off, values=v.values, val_off=v.val_off, flags=v.flags, n=k,
                         key_bytes=self.ko[k], value_bytes=self.vo[k])


class Index:
    """order / pfx / result buffers of `cap` words and the two calls into them, on torch's current stream."""

    def __init__(self, cap):
        self.order, self.pfx = (torch.zeros(max(cap, 1), dtype=torch.int64, device="cuda") for _ in range(2))
        self.result = torch.zeros(WORDS, dtype=torch.int64, device="cuda")

    def _st(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def build(self, view, bound):
        rc = L.lib().rio_mem_index_build(L.default_ctx(0), ctypes.addressof(view), bound, self.order.data_ptr(),
                                         self.pfx.data_ptr(), self.result.data_ptr(), self._st())
        assert rc == L.RIO_OK, rc
        return self

    def extend(self, view, n_old, bound):
        rc = L.lib().rio_mem_index_extend(L.default_ctx(0), ctypes.addressof(view), n_old, bound, self.order.data_ptr(),
                                          self.pfx.data_ptr(), self.result.data_ptr(), self._st())
        assert rc == L.RIO_OK, rc
        return self

    def read(self):
        """(result words, order[:n_keys], pfx[:n_keys])."""
        torch.cuda.synchronize()
        words = [x & _NONE for x in self.result.cpu().tolist()]
        nk = words[L.RIO_MERGE_R_N_OUT]
        assert nk <= self.order.numel()
        return (words, [x & _NONE for x in self.order[:nk].cpu().tolist()], [x & _NONE for x in self.pfx[:nk].cpu().tolist()])


def model_index(ops):
    """What the index of `ops` holds, from a dict and sorted()."""
    latest = {}
    for i, (k, _) in enumerate(ops):
        latest[k] = i
    keys = sorted(latest)
    words = [0] * WORDS
    words[L.RIO_MERGE_R_N_OUT] = len(keys)
    words[L.RIO_MERGE_R_VALUE_BYTES] = sum(len(ops[latest[k]][1] or b"") for k in keys)
    words[L.RIO_MERGE_R_NULL_VALUES] = sum(ops[latest[k]][1] is None for k in keys)
    words[L.RIO_MERGE_R_KEY_BYTES] = sum(len(k) for k in keys)
    words[L.RIO_MERGE_R_FIRST_DUP] = words[L.RIO_MERGE_R_UNSORTED] = _NONE
    return words, [latest[k] for k in keys], [int.from_bytes(k[:8].ljust(8, b"\0"), "big") for k in keys]


def extend_equals_build(ops, cuts):
    """An empty index extended at every cut of `ops` (ascending op counts): after each step it is the build of that
    prefix (separate buffers; its bound is the prefix's longest key, the extend's the new ops' alone) and the model's."""
    log = Log(ops)
    got = Index(len(ops)).build(log.view(0), 0)
    prev = 0
    for cut in cuts:
        got.extend(log.view(cut), prev, log.bound(prev, cut))
        want = Index(cut).build(log.view(cut), log.bound(0, cut)).read()
        assert got.read() == want, (prev, cut)
        assert want == model_index(ops[:cut]), cut
        prev = cut


# ---- 1. places of a tail key --------------------------------------------------------------------------------------

OLD = [(b"k%02d" % i, b"v%d" % i) for i in range(2, 21, 2)]
OLD_T = OLD + [(b"k06", None)]  # with an old tombstone
PLACES = {
    "below all": (OLD, [(b"a", b"new")]),
    "above all": (OLD, [(b"k99", b"new")]),
    "the first gap": (OLD, [(b"k03", b"new")]),
    "a middle gap": (OLD, [(b"k11", b"new")]),
    "the last gap": (OLD, [(b"k19", b"new")]),
    "a gap by a longer key": (OLD, [(b"k10\0", b"new")]),
    "a gap by a shorter key": (OLD, [(b"k1", b"new")]),
    "the first key again": (OLD, [(b"k02", b"rewritten")]),
    "a middle key again": (OLD, [(b"k10", b"")]),
    "the last key again": (OLD, [(b"k20", b"rewritten, and longer")]),
    "a key as a tombstone": (OLD, [(b"k10", None)]),
    "a new key as a tombstone": (OLD, [(b"k11", None)]),
    "an old tombstone revived": (OLD_T, [(b"k06", b"back")]),
    "an old tombstone again": (OLD_T, [(b"k06", None)]),
    "three keys in one gap": (OLD, [(b"k11b", b"3"), (b"k11", b"1"), (b"k11a", None)]),
    "every old key again": (OLD_T, [(k, b"again-" + k) for k, _ in OLD[::-1]]),
    "put delete put inside the tail": (OLD, [(b"k11", b"1"), (b"k11", None), (b"k11", b"3"), (b"k04", None), (b"k04", b"x")]),
    "new first, new last and rewrites": (OLD, [(b"zz", b"l"), (b"k08", b"r"), (b"", b"the empty key"), (b"k02", None)]),
    "n_old = 0": ([], OLD_T),
    "n_old = ops.n": (OLD_T, []),
    "an empty log and an empty tail": ([], []),
    "one old op": ([(b"k", b"v")], [(b"k", None), (b"j", b"w")]),
}


@pytest.mark.parametrize("name", list(PLACES))
def test_places_of_a_tail_key(name):
    old, tail = PLACES[name]
    extend_equals_build(old + tail, [len(old), len(old) + len(tail)])


# ---- 2. key shapes ------------------------------------------------------------------------------------------------

LONG = b"L" * (MAXK - 1)
FORMS = [b"a", b"a\0", b"a\0\0", b"ab", b"abc\0\0\0\0", b"ab\0\0\0\0\0\0", b"ab\0\0\0\0\0\0\0", P8, P8 + b"\0", P8 + b"x",
         P8 + b"y", P8 + b"xx", P8 + b"xxlong-tail-A", P8 + b"xxlong-tail-B", b"prefix_", b"\xfe\xff", LONG + b"x", b""]
SHAPES = {
    "even forms old, odd forms new": (FORMS[::2], FORMS[1::2]),
    "odd forms old, even forms new": (FORMS[1::2], FORMS[::2]),
    "every form on both sides": (FORMS, FORMS[::-1]),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_key_shapes_across_the_cut(name):
    assert len(LONG + b"x") == MAXK
    old, new = SHAPES[name]
    ops = [(k, b"old:" + k[:12]) for k in old] + [(k, None if i % 5 == 4 else b"new:" + k[:9]) for i, k in enumerate(new)]
    extend_equals_build(ops, [len(old), len(ops)])


# ---- 3. chains ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [21, 22, 23, 24, 25])
def test_chains_of_extends(seed):
    rng = random.Random(seed)
    keys = [b"key-%03d" % i + b"-tail" * (i % 3) for i in range(60)]
    ops = [(rng.choice(keys), None if rng.randrange(4) == 0 else bytes(rng.randrange(256) for _ in range(rng.choice([0, 1, 7, 33]))))
           for _ in range(300)]
    cuts = sorted(rng.sample(range(1, 300), 6)) + [300]
    extend_equals_build(ops, cuts)


# ---- 4. round the grid again --------------------------------------------------------------------------------------

BIG = 2048 * 256 + 3


def _big_log(n_front, front_keys, back_keys):
    """A log of 4-byte big-endian keys (uint32 arrays), values of i % 3 bytes, no tombstones but op 1 of the back part;
    returns (DeviceOps, key_off, val_off) without going through Python lists of bytes."""
    k = np.concatenate([front_keys, back_keys]).astype(">u4")
    n = len(k)
    vlen = np.arange(n, dtype=np.int64) % 3
    flags = np.zeros(n + 1, dtype=np.uint8)
    flags[n_front + 1] = L.RIO_FLAG_NIL
    vlen[n_front + 1] = 0
    ko, vo = np.arange(n + 1, dtype=np.int64) * 4, np.concatenate([[0], np.cumsum(vlen)]).astype(np.int64)
    keys = np.concatenate([k.view(np.uint8), np.zeros(L.RIO_DEVICE_PAD, dtype=np.uint8)])
    values = np.full(int(vo[-1]) + L.RIO_DEVICE_PAD, 0x76, dtype=np.uint8)
    up = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    dev = M.DeviceOps(0, up(keys), up(ko), up(values), up(vo), up(flags), n, 4 * n, int(vo[-1]), 4)
    return dev, ko, vo, k.astype(np.int64), vlen, flags


@pytest.mark.parametrize("shape", ["five ops behind many", "many ops behind five"])
def test_more_entries_than_one_grid(shape):
    rng = np.random.default_rng(4)
    many = (rng.permutation(BIG).astype(np.int64) + 10) * 2  # distinct, even, unordered
    five = np.array([7, 0xFFFFFFF0, many[0], many[BIG // 2], many[BIG - 1]])  # a new first, a new last, three rewrites
    front, back = (many, five) if shape.startswith("five") else (five, many)
    dev, ko, vo, k, vlen, flags = _big_log(len(front), front, back)
    n_old, n = len(front), len(front) + len(back)
    v = dev.view
    old = L.OpsView(keys=v.keys, key_off=v.key_off, values=v.values, val_off=v.val_off, flags=v.flags, n=n_old,
                    key_bytes=int(ko[n_old]), value_bytes=int(vo[n_old]))
    got = Index(n).build(old, 4).extend(v, n_old, 4).read()
    want = Index(n).build(v, 4).read()
    assert got == want
    latest = dict(zip(k.tolist(), range(n)))  # the later op of a key replaces the earlier one
    ks = sorted(latest)
    order = [latest[x] for x in ks]
    assert len(ks) == BIG + 2 and want[1] == order and want[2] == [x << 32 for x in ks]
    words = want[0]
    assert words[L.RIO_MERGE_R_N_OUT] == BIG + 2 and words[L.RIO_MERGE_R_KEY_BYTES] == 4 * (BIG + 2)
    assert words[L.RIO_MERGE_R_VALUE_BYTES] == int(vlen[order].sum()) and words[L.RIO_MERGE_R_NULL_VALUES] == int(flags[order].sum())


# ---- 5. rejection -------------------------------------------------------------------------------------------------

def test_a_rejected_tail_op_and_a_rejected_old_index():
    ops = [(b"ab", b"1"), (b"abc", b"2"), (b"a", b"3"), (b"abcd", b"4"), (b"b", b"5"), (b"abcde", b"6"), (b"c", b"7")]
    log = Log(ops)
    # tail op j = 2 (op 5 of the log) is one byte over the tail's bound
    idx = Index(len(ops)).build(log.view(3), 3).extend(log.view(7), 3, 4)
    words, order, _ = idx.read()
    assert words[L.RIO_MERGE_R_UNSORTED] == 3 + 2 and words[L.RIO_MERGE_R_N_OUT] == 0 and order == []
    # an old index rejected at op 1 (a bound of 2 for a key of 3) stays rejected with its op after a good tail
    idx = Index(len(ops)).build(log.view(3), 2)
    assert idx.read()[0][L.RIO_MERGE_R_UNSORTED] == 1
    words, order, _ = idx.extend(log.view(7), 3, 5).read()
    assert words[L.RIO_MERGE_R_UNSORTED] == 1 and words[L.RIO_MERGE_R_N_OUT] == 0 and order == []
    # ... and after another extend; only the build over the whole log clears it
    words = idx.extend(log.view(7), 5, 5).read()[0]
    assert words[L.RIO_MERGE_R_UNSORTED] == 1 and words[L.RIO_MERGE_R_N_OUT] == 0
    assert idx.build(log.view(7), 5).read() == model_index(ops)


def test_the_mirror_keeps_a_rejection_until_rebuild():
    ops = [(b"ab", b"1"), (b"abc", b"2"), (b"a", b"3"), (b"b", b"4"), (b"c", None)]
    log = Log(ops)
    v3, v5 = log.view(3), log.view(5)
    d = log.dev
    short = M.DeviceOps(0, d.keys, d.key_off, d.values, d.val_off, d.flags, 3, v3.key_bytes, v3.value_bytes, 2)  # a bound that lies
    longer = M.DeviceOps(0, d.keys, d.key_off, d.values, d.val_off, d.flags, 5, v5.key_bytes, v5.value_bytes, 2)
    idx = M.DeviceMemIndex(short)
    assert idx.rejected() is not None and idx.result_words()[L.RIO_MERGE_R_UNSORTED] == 1
    assert idx.extend(longer) is idx and idx.ops is longer
    assert "op 1 of the log" in str(idx.rejected()) and idx.n_keys() == 0
    assert all(e is not None for _, e in idx.GetBatch([b"a", b"b"]))
    idx.rebuild(log.dev)  # the log with its true bound
    assert idx.rejected() is None and idx.n_keys() == 5
    assert idx.GetBatch([b"a", b"c", b"abc"]) == [(b"3", None), (None, M.KeyTombstoned), (b"2", None)]


# ---- 6. clamps ----------------------------------------------------------------------------------------------------

def test_hostile_order_words_and_counts_stay_in_range():
    """The old index's n_keys word above n_old and old order words at and above n_old, handed to the extend: the call
    returns and every order word it leaves names an op of the log. Nothing else is asserted."""
    ops = [(b"k%d" % i, b"v%d" % i) for i in range(8)] + [(b"k3", b"again"), (b"j", b"new"), (b"k9", None)]
    log = Log(ops)
    n_old, n = 8, len(ops)
    idx = Index(n).build(log.view(n_old), 2)
    torch.cuda.synchronize()
    idx.result[L.RIO_MERGE_R_N_OUT] = n_old + 5000
    idx.order[1], idx.order[3], idx.order[6] = n_old, n_old + 1000, n
    idx.extend(log.view(n), n_old, 2)
    torch.cuda.synchronize()
    assert all(0 <= w < n for w in idx.order.cpu().tolist())


# ---- 7. rio_ops_append --------------------------------------------------------------------------------------------

FIRST = [(b"k%02d" % i, b"v%d" % i) for i in range(20)]
MORE = [(b"k03", b"overwritten"), (b"k05", None), (b"k20", b"added"), (b"a-new-first", b"x"), (b"k07", b""), (b"k05", b"back")]
LAST = [(b"empty-value", b""), (b"k01", None)]


def _arrays(ops):
    """(keys, key_off, values, val_off, flags) of a device log (DeviceOps or DeviceOpLog) over its n ops, on the host."""
    v = ops.view
    torch.cuda.synchronize()
    return (bytes(ops.keys[:v.key_bytes].cpu().numpy()), ops.key_off[:v.n + 1].cpu().tolist(),
            bytes(ops.values[:v.value_bytes].cpu().numpy()), ops.val_off[:v.n + 1].cpu().tolist(), ops.flags[:v.n].cpu().tolist())


@pytest.mark.parametrize("caps", [dict(), dict(ops_cap=4, keys_cap=L.RIO_DEVICE_PAD, values_cap=L.RIO_DEVICE_PAD + 1)],
                         ids=["spare room", "a capacity that forces doubling"])
def test_ops_append_is_the_upload_of_the_concatenation(caps):
    log = M.DeviceOpLog(0, **caps)
    with torch.cuda.device(0):
        second = _batch(MORE).upload(0)  # a batch that is on the device already
    third = M.DeviceOpLog(0).append(_batch(LAST))
    for batch in (_batch(FIRST), second, _batch([]), third):  # an empty batch in between changes nothing
        assert log.append(batch) is log
    want = Log(FIRST + MORE + LAST)
    assert _arrays(log) == _arrays(want.dev)
    v = log.view
    assert (v.n, v.key_bytes, v.value_bytes) == (28, want.ko[-1], want.vo[-1]) and log.max_key_len == len(b"empty-value")
    assert log.ops_cap >= 28 and log.keys_cap >= v.key_bytes + L.RIO_DEVICE_PAD and log.values_cap >= v.value_bytes + L.RIO_DEVICE_PAD
    assert log.key_off.numel() == log.ops_cap + 1 and log.keys.numel() == log.keys_cap
    # the host path writes the same arrays
    host = M.DeviceOpLog(0, **caps)
    for ops in (FIRST, MORE, LAST):
        w = Log(ops)
        host.append_host(b"".join(k for k, _ in ops), w.ko, b"".join(v or b"" for _, v in ops), w.vo,
                         bytes(L.RIO_FLAG_NIL if v is None else 0 for _, v in ops))
    assert _arrays(host) == _arrays(want.dev) and host.max_key_len == log.max_key_len
    # and the index of the appended log is the index of the uploaded one
    assert Index(28).build(v, log.max_key_len).read() == model_index(FIRST + MORE + LAST)


# ---- 8. end to end without the host -------------------------------------------------------------------------------

def test_batches_applied_on_the_device_are_read_and_flushed(tmp_path):
    a = _appender(str(tmp_path / "wal"))
    tables = [{b"k01": b"table-old", b"k05": b"table-5", b"t-only": b"t"}, {b"k01": b"table-new", b"k20": b"hidden", b"nil": None}]
    sr = open_stack(tmp_path, tables)
    store, model = M.DeviceMemStore(0, ops_cap=8, keys_cap=128, values_cap=128), dm.ModelStore()
    host = M.NewMemStore()  # fed the same ops through its point calls
    view = DB.DBReadView(sr, store)
    queries = [k for k, _ in FIRST] + [b"k20", b"a-new-first", b"absent", b"t-only", b"nil", b"empty-value"]
    assert store.Size() == 0 and store.Get(b"k01") == (None, M.KeyNotFound)
    first_index = store._index()
    for ops in (FIRST, MORE, LAST):
        dev_ops, err = DB.append_batch(a, _batch(ops))
        assert err is None, err
        assert store.Apply(dev_ops) is None
        apply(host, model, ops)
        check(view, tables, model, None, queries)
        assert store.Size() == host.Size() == len(model.latest)
        check_index(store, model)
    assert store._index() is first_index and store.log.n == 28
    assert store.ContainsBatch([b"k05", b"k01", b"zz"]) == [True, False, False] and store.Contains(b"k07") is True  # empty, not nil
    assert a.Close() is None
    for name, call in (("with", "FlushWithTombstones"), ("without", "Flush")):
        d_base, h_base = str(tmp_path / f"dev-{name}"), str(tmp_path / f"host-{name}")
        assert getattr(store, call)(S.WriteBasePath(d_base)) is None
        assert getattr(host, call)(S.WriteBasePath(h_base)) is None
        files = sorted(os.listdir(h_base))
        assert files == sorted(os.listdir(d_base)) and len(files) >= 3
        for f in files:
            assert open(os.path.join(d_base, f), "rb").read() == open(os.path.join(h_base, f), "rb").read(), f
    assert store.Flush() is not None  # basePath was not supplied
    view.Close()
    sr._free_stack()


# ---- 9. MemStore --------------------------------------------------------------------------------------------------

def test_a_memstore_that_grows_extends_its_index(monkeypatch):
    ms, model = M.NewMemStore(), dm.ModelStore()
    apply(ms, model, FIRST)
    queries = [k for k, _ in FIRST] + [b"k20", b"a-new-first", b"absent"]
    same(ms.GetBatch(queries), [ms.Get(q) for q in queries])
    first_index = ms._index()
    apply(ms, model, MORE)
    lib, calls = L.lib(), []

    def counted(name):
        real = getattr(lib, name)

        def call(*args):
            calls.append(name)
            return real(*args)

        return call

    for name in ("rio_mem_index_build", "rio_mem_index_extend"):
        monkeypatch.setattr(lib, name, counted(name))
    assert ms._index() is first_index
    assert calls == ["rio_mem_index_extend"]
    assert ms._index() is first_index and calls == ["rio_mem_index_extend"]  # nothing new: nothing runs
    monkeypatch.undo()
    assert first_index.ops.n == len(FIRST) + len(MORE)
    check_index(ms, model)
    same(ms.GetBatch(queries), [ms.Get(q) for q in queries])
    # a store that doubles its device arrays on the way (1024 ops and 64 KiB to begin with)
    big = [(b"key-%05d" % (i * 7919 % 1500), b"v" * (i % 150)) for i in range(1200)]
    apply(ms, model, big)
    check_index(ms, model)
    assert ms._dev_log.ops_cap == 2048 and ms._dev_log.values_cap == 1 << 17 and ms._index() is first_index
