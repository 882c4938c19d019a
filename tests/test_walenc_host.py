"""Batched writes, the parts that need no GPU: the model the GPU tests compare with against google.protobuf (where
it imports: the message class of test_wal_mutation_host.py), the argument errors of rio_wal_ops_encode, which
return before any device call, wal.batch_cuts against the record-by-record loop, FileWriter.WriteFramed and
wal.Appender.AppendFramed from host-built images against the loops of Write and Append, and WriteBatch."""
import ctypes
import os
import random

import numpy as np
import pytest

import recordio as R
import sstables as S
import wal as W
import walenc_model as EM
from recordio import _lib as L
from recordio.writer import encode_file
from simpledb import proto as P

BOUNDARY = (0, 1, 127, 128, 16383, 16384)


# ---- the model -------------------------------------------------------------------------------------------

def test_model_fixed_bytes():
    e = EM.expected([EM.put(b"k", b"vv"), EM.delete(b"key", b"hidden"), EM.put(b"", b""), EM.delete(b""), EM.put(b"k", b"")])
    assert e["records"] == [bytes.fromhex("0a07" "1a016b" "22027676"), bytes.fromhex("1205" "12036b6579"), b"\x0a\x00",
                            b"\x12\x00", bytes.fromhex("0a03" "1a016b")]
    assert e["rec_off"] == [0, 9, 16, 18, 20, 25] and e["result"] == [5, 25, 3, 2, 3, EM.NONE, 0, 0]
    assert EM.expected([])["result"] == [0, 0, 0, 0, 0, EM.NONE, 0, 0] and EM.expected([])["rec_off"] == [0]
    k, ko, v, vo, fl = EM.arrays([EM.put(b"ab", b"1"), EM.delete(b"c", b"xyz"), EM.put(b"", b"22")])
    assert (k, v) == (b"abc", b"1xyz22") and ko.tolist() == [0, 2, 3, 3] and vo.tolist() == [0, 1, 4, 6]
    assert fl.tolist() == [0, L.RIO_FLAG_NIL, 0]
    assert EM.first_bad(ko, vo, 3, 6) == EM.NONE and EM.first_bad(ko, vo, 2, 6) == 1 and EM.first_bad(ko, vo, 3, 5) == 2
    assert EM.first_bad([0, 2, 1, 3], vo, 3, 6) == 1


def test_model_body_lengths_at_the_varint_boundaries():
    # the body of an upsert is field(klen) + field(vlen); with a 16-byte key the key field takes 18 bytes
    for body in (127, 128, 16383, 16384, (1 << 21) - 1, 1 << 21):
        rest = body - 18
        vlen = next(v for v in range(rest - 5, rest) if EM.field_len(v) == rest)
        op = EM.put(b"K" * 16, b"v" * vlen)
        assert EM.body_len(op) == body
        assert len(EM.record(op)) == 1 + len(P.put_varint(body)) + body
    for klen in (125, 126):  # a delete's body 127 and 128
        assert EM.body_len(EM.delete(b"k" * klen)) == klen + 2
    assert (EM.body_len(EM.delete(b"k" * 125)), EM.body_len(EM.delete(b"k" * 126))) == (127, 128)


def _by_protobuf(cls, op):
    key, value, nil = op
    m = cls()
    if nil:
        m.deleteTombStone.SetInParent()
        m.deleteTombStone.keyBytes = key
    else:
        m.addition.SetInParent()
        m.addition.keyBytes = key
        m.addition.valueBytes = value
    return m.SerializeToString(deterministic=True)


def test_model_agrees_with_protobuf():
    from test_wal_mutation_host import _message_class

    cls = _message_class()
    ops = EM.corpus(2025, 300)
    ops += [EM.put(b"k" * a, b"v" * b) for a in BOUNDARY for b in BOUNDARY] + [EM.delete(b"k" * a, b"hid") for a in BOUNDARY]
    ops += [EM.put(b"key", b"v" * n) for n in ((1 << 21) - 1, 1 << 21)]
    for op in ops:
        assert EM.record(op) == _by_protobuf(cls, op), (len(op[0]), len(op[1]), op[2])


# ---- rio_wal_ops_encode: argument errors -----------------------------------------------------------------

def test_encode_argument_errors_return_before_any_device_call():
    lib = L.lib()
    # As in test_memstore_host.py: no context can be created without a device, so ctx is a placeholder that is
    # never read: the entry point checks its arguments before the first read of *ctx.
    page = ctypes.create_string_buffer(1 << 16)
    ctx = ctypes.addressof(page)
    buf = ctypes.addressof(ctypes.create_string_buffer(64))
    enc = lib.rio_wal_ops_encode
    fields = ("keys", "key_off", "values", "val_off", "flags")
    view = L.OpsView(n=0)
    v = ctypes.addressof(view)
    assert enc(None, v, buf, 64, buf, buf, None) == L.RIO_ERR_ARG
    assert enc(ctx, None, buf, 64, buf, buf, None) == L.RIO_ERR_ARG
    assert enc(ctx, v, buf, 64, None, buf, None) == L.RIO_ERR_ARG
    assert enc(ctx, v, buf, 64, buf, None, None) == L.RIO_ERR_ARG
    assert enc(ctx, v, None, 1, buf, buf, None) == L.RIO_ERR_ARG  # no arena for a capacity
    view.n = 1
    for missing in fields:
        for f in fields:
            setattr(view, f, None if f == missing else buf)
        assert enc(ctx, v, buf, 64, buf, buf, None) == L.RIO_ERR_ARG, missing
    for f in fields:
        setattr(view, f, buf)
    view.n = (1 << 31) - 1
    assert enc(ctx, v, buf, 64, buf, buf, None) == L.RIO_ERR_UNSUPPORTED
    assert lib.rio_wal_ops_encode_bound(0, 0, 0) == 0
    assert lib.rio_wal_ops_encode_bound(3, 10, 100) == 110 + 33 * 3
    # the bound holds for the longest headers there are: three 10-byte varints need lengths no arena has, so the
    # largest record the tests build, and every boundary, stays below it
    for op in [EM.put(b"k" * a, b"v" * b) for a in BOUNDARY for b in BOUNDARY] + [EM.delete(b"k" * a) for a in BOUNDARY]:
        assert len(EM.record(op)) <= lib.rio_wal_ops_encode_bound(1, len(op[0]), 0 if op[2] else len(op[1]))
    assert lib.rio_writer_append_framed(None, buf, 1) == L.RIO_ERR_STATE


# ---- wal.batch_cuts --------------------------------------------------------------------------------------

def _cuts_agree(size0, raw, framed, max_size):
    got = W.batch_cuts(size0, raw, framed, max_size)
    assert got == EM.batch_cuts_loop(size0, list(raw), list(framed), max_size), (size0, max_size)
    assert all(isinstance(c, int) for c in got)
    return got


def test_batch_cuts_edges():
    assert _cuts_agree(8, [], [], 100) == []
    assert _cuts_agree(500, [], [], 100) == []
    raw, framed = [10, 10, 10, 10], [15, 15, 15, 15]
    # the running size before record 2 is 8 + 30 = 38: max_size below, at and one above size + raw
    assert _cuts_agree(8, raw, framed, 47) == [2]
    assert _cuts_agree(8, raw, framed, 48) == [3]
    assert _cuts_agree(8, raw, framed, 49) == [3]
    # an oversize first record leaves a header-only file behind it, and is checked once
    assert _cuts_agree(8, [1000, 10, 10], [1005, 15, 15], 100) == [0, 1]
    # an oversize middle record opens a file, and the record after it the next
    assert _cuts_agree(8, [10, 1000, 10, 10], [15, 1005, 15, 15], 100) == [1, 2]
    # framed below raw (Snappy): the raw length decides the check, the framed length the growth
    assert _cuts_agree(8, [60, 60, 60, 60, 60], [20, 20, 20, 20, 20], 100) == [2, 4]
    # a part-filled current file
    assert _cuts_agree(90, [10, 10], [15, 15], 100) == [1]
    assert _cuts_agree(91, [10, 10], [15, 15], 100) == [0]
    assert _cuts_agree(10 ** 6, [1], [6], 100) == [0]
    # every record oversize: a file each
    assert _cuts_agree(8, [200] * 5, [205] * 5, 100) == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("seed", range(6))
def test_batch_cuts_seeded(seed):
    rng = np.random.default_rng(seed)
    n = (3000, 5000, 1, 2500, 4097, 1024)[seed]
    raw = rng.integers(0, 400, n)
    if seed % 2:
        raw[rng.integers(0, n, 5)] = 5000  # oversize records
    framed = np.where(rng.random(n) < 0.5, raw // 3 + 6, raw + 7)  # compressed below raw, or raw plus a header
    for max_size in (64, 1000, 4096, 1 << 20):
        for size0 in (8, 700, max_size, max_size + 1):
            got = _cuts_agree(size0, raw, framed, max_size)
            if max_size == 1 << 20 and size0 == 8:
                assert len(got) <= 1
    # files longer than the first search window (1024 records): small records, a large limit
    small = np.full(10000, 3)
    assert len(_cuts_agree(8, small, small + 5, 40000)) == 2


# ---- FileWriter.WriteFramed / Appender.AppendFramed ------------------------------------------------------

def _records(seed, n=300):
    return [EM.record(op) for op in EM.corpus(seed, n)]


def _framed(records, comp):
    """The v4 image of the records, every record's offset in it, and the raw lengths."""
    img = encode_file(records, comp)
    lens = [len(encode_file([r], comp)) - 8 for r in records]
    off = np.cumsum([8] + lens)
    assert off[-1] == len(img)
    return img, off[:-1], [len(r) for r in records]


@pytest.mark.parametrize("comp", [L.COMP_NONE, L.COMP_SNAPPY])
def test_write_framed_equals_the_write_loop(tmp_path, comp):
    recs = _records(1)
    a, b = str(tmp_path / "a.rio"), str(tmp_path / "b.rio")
    w, _ = R.NewFileWriter(a, comp)
    assert w.Open() is None
    for r in recs:
        assert w.Write(r)[1] is None
    size = w.Size()
    assert w.Close() is None
    img, off, _ = _framed(recs, comp)
    w, _ = R.NewFileWriter(b, comp)
    assert w.Open() is None and w.Size() == 8
    cut = int(off[100])
    assert w.WriteFramed(img[8:cut]) is None and w.Size() == cut
    assert w.WriteFramed(b"") is None and w.Size() == cut
    assert w.WriteFramed(memoryview(img)[cut:]) is None and w.Size() == len(img) == size
    assert w.Close() is None
    assert open(a, "rb").read() == open(b, "rb").read() == img


def _appender(path, comp, max_size):
    os.makedirs(path)
    opts, err = W.NewWriteAheadLogOptions(W.BasePath(path), W.MaximumWalFileSizeBytes(max_size),
                                          W.WriterFactory(lambda p: R.NewFileWriter(p, comp)))
    assert err is None, err
    a, err = W.NewAppender(opts)
    assert err is None, err
    return a


def _snapshot(d):
    return {name: open(os.path.join(d, name), "rb").read() for name in sorted(os.listdir(d))}


@pytest.mark.parametrize("comp", [L.COMP_NONE, L.COMP_SNAPPY])
@pytest.mark.parametrize("max_size", [100, 2000, 1 << 20])
def test_append_framed_equals_the_append_loop(tmp_path, comp, max_size):
    first, second, third = _records(2, 40), _records(3, 300), _records(4, 120)
    second[150] = P.marshal_upsert(b"big", bytes(3000))  # compresses far below its raw length; oversize for 100 and 2000
    want, got = _appender(str(tmp_path / "want"), comp, max_size), _appender(str(tmp_path / "got"), comp, max_size)
    for r in first + second + third:
        assert want.Append(r) is None
    assert want.Close() is None
    for r in first:  # a part-filled current file before the first batch
        assert got.Append(r) is None
    assert got.AppendFramed(*_framed(second, comp)) is None
    assert got.AppendFramed(*_framed([], comp)) is None
    assert got.AppendFramed(*_framed(third, comp)) is None
    assert got.nextWriterNumber == want.nextWriterNumber and got.currentWriter.Size() > 8
    assert got.Close() is None
    a, b = _snapshot(str(tmp_path / "want")), _snapshot(str(tmp_path / "got"))
    assert list(a) == list(b) and a == b
    assert len(a) == 1 if max_size == 1 << 20 else len(a) >= 3


def test_append_framed_refusals(tmp_path):
    recs = _records(5, 10)
    a = _appender(str(tmp_path / "gz"), L.COMP_GZIP, 1 << 20)
    assert isinstance(a.AppendFramed(*_framed(recs, L.COMP_NONE)), S.UnsupportedError)
    a = _appender(str(tmp_path / "none"), L.COMP_NONE, 1 << 20)
    assert isinstance(a.AppendFramed(*_framed(recs, L.COMP_SNAPPY)), S.UnsupportedError)  # another compression's image
    a.currentWriter = object()
    assert isinstance(a.AppendFramed(*_framed(recs, L.COMP_NONE)), S.UnsupportedError)
    # the one-million-file error comes back through Rotate, as under Append
    a = _appender(str(tmp_path / "full"), L.COMP_NONE, 50)
    a.nextWriterNumber = 1000000
    err = a.AppendFramed(*_framed([b"x" * 100], L.COMP_NONE))
    assert err is not None and "not supporting more than one million wal files" in str(err)
    assert str(err).startswith("error while rotating wal writer '")


# ---- WriteBatch ------------------------------------------------------------------------------------------

def test_write_batch_holds_the_op_log():
    import simpledb as DB

    b = DB.WriteBatch()
    assert len(b) == 0
    assert b.PutBytes(b"k1", b"v1") is None and b.DeleteBytes(b"k1") is None
    assert b.PutBytes(b"", b"") is None and b.DeleteBytes(b"") is None and b.PutBytes(None, None) is None
    assert b.Put("", "v") is DB.ErrEmptyKeyValue and b.Put("k", "") is DB.ErrEmptyKeyValue
    assert str(DB.ErrEmptyKeyValue) == "neither empty keys nor values are allowed"
    assert b.Put("schlüssel", "wert") is None and b.Delete("schlüssel") is None and b.Delete("") is None
    assert len(b) == 8
    ks = "schlüssel".encode()
    ops = [EM.put(b"k1", b"v1"), EM.delete(b"k1"), EM.put(b"", b""), EM.delete(b""), EM.put(b"", b""), EM.put(ks, b"wert"),
           EM.delete(ks), EM.delete(b"")]
    k, ko, v, vo, fl = EM.arrays(ops)
    assert (bytes(b._keys), bytes(b._values), bytes(b._flags)) == (k, v, fl.tobytes())
    assert b._key_off == ko.tolist() and b._val_off == vo.tolist() and b._max_key_len == len(ks)
    # the same arrays a MemStore keeps for the same calls
    import memstore as MS

    m = MS.NewMemStore()
    m.Upsert(b"k1", b"v1"), m.Tombstone(b"k1"), m.Upsert(ks, b"wert"), m.Tombstone(ks)
    b2 = DB.WriteBatch()
    b2.PutBytes(b"k1", b"v1"), b2.DeleteBytes(b"k1"), b2.Put("schlüssel", "wert"), b2.Delete("schlüssel")
    for name in ("_keys", "_values", "_key_off", "_val_off", "_flags", "_max_key_len"):
        assert getattr(m, name) == getattr(b2, name), name
