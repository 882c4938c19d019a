"""Batched writes on the device (GPU): rio_wal_ops_encode against walenc_model (every op through
simpledb.proto.marshal_upsert / marshal_delete), and simpledb.append_batch end to end against the host loop of
marshal + Append and against recover_wal. Every case compares rec_off, the result block and the record arena byte
for byte with the model; the fill bytes behind the records, up to CANARY bytes past the capacity, stay untouched."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

import flush_model as FM
import memstore as MS
import recordio as R
import simpledb as DB
import wal as W
import walenc_model as EM
from conftest import PKG
from recordio import _lib as L
from simpledb import proto as P

pytestmark = pytest.mark.gpu

_NONE = 0xFFFFFFFFFFFFFFFF
_SRC = open(os.path.join(PKG, "csrc", "rio_walenc.hip")).read()
GRID_CAP = int(re.search(r"kWalEncGridCap = (\d+);", _SRC).group(1))
COPY_GRID_CAP = int(re.search(r"kWalEncCopyGridCap = (\d+);", _SRC).group(1))
LONG_ITEM = int(re.search(r"kWalEncLongItem = (\d+);", _SRC).group(1))
CANARY, FILL = 64, 0xA5


def ctx():
    return L.default_ctx(0)


class Log:
    """An op log in device memory as rio_ops_view takes it, from the model's host arrays."""

    def __init__(self, ops=None, arrays=None, key_bytes=None, value_bytes=None):
        keys, key_off, values, val_off, flags = arrays if arrays is not None else EM.arrays(ops)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()  # noqa: E731
        pad = np.zeros(L.RIO_DEVICE_PAD, dtype=np.uint8)
        self.n = len(flags)
        self.t = dict(keys=up(np.concatenate([np.frombuffer(keys, dtype=np.uint8), pad]), np.uint8), key_off=up(key_off, np.int64),
                      values=up(np.concatenate([np.frombuffer(values, dtype=np.uint8), pad]), np.uint8),
                      val_off=up(val_off, np.int64), flags=up(np.concatenate([flags, pad[:1]]), np.uint8))
        self.key_bytes = len(keys) if key_bytes is None else key_bytes
        self.value_bytes = len(values) if value_bytes is None else value_bytes
        self.view = L.OpsView(n=self.n, key_bytes=self.key_bytes, value_bytes=self.value_bytes,
                              **{k: v.data_ptr() for k, v in self.t.items()})

    def bound(self):
        return int(L.lib().rio_wal_ops_encode_bound(self.n, self.key_bytes, self.value_bytes))


class Out:
    """The outputs of one call, filled beforehand: cap + CANARY record bytes, n + 1 offsets, the result block."""

    def __init__(self, n, cap):
        self.n, self.cap = n, cap
        self.records = torch.full((cap + CANARY,), FILL, dtype=torch.uint8, device="cuda")
        self.rec_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        self.res = torch.full((L.RIO_WALENC_RESULT_WORDS,), -1, dtype=torch.int64, device="cuda")

    def launch(self, log, st):
        rc = L.lib().rio_wal_ops_encode(ctx(), ctypes.addressof(log.view), self.records.data_ptr(), self.cap,
                                        self.rec_off.data_ptr(), self.res.data_ptr(), st)
        assert rc == L.RIO_OK, rc

    def read(self):
        return (self.rec_off.cpu().tolist(), [x & _NONE for x in self.res.cpu().tolist()],
                self.records.cpu().numpy().tobytes())


def encode(log, cap=None):
    """One call on a stream of the caller's -> rec_off, result, the arena with its CANARY bytes."""
    out = Out(log.n, log.bound() if cap is None else cap)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        out.launch(log, ctypes.c_void_p(st.cuda_stream))
    st.synchronize()
    return out.read()


def check(ops, log=None):
    """The ops through the device against the model, with the bound as capacity; -> the model."""
    want = EM.expected(ops)
    log = log or Log(ops)
    rec_off, res, arena = encode(log)
    assert res == want["result"]
    assert rec_off == want["rec_off"]
    total = rec_off[-1]
    assert total <= log.bound()
    assert arena[:total] == want["arena"]
    assert arena[total:] == bytes([FILL]) * (log.bound() + CANARY - total)
    return want


# ---- op counts -------------------------------------------------------------------------------------------

def _tiny_ops(n, seed):
    pool = [EM.put(bytes([c]), v) for c in range(97, 123) for v in (b"", b"v")] + [EM.delete(bytes([c])) for c in range(97, 123)]
    picks = np.random.default_rng(seed).integers(0, len(pool), n).tolist()
    return [pool[i] for i in picks]


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_op_counts(n):
    want = check(_tiny_ops(n, n))
    assert want["result"][0] == n
    if n >= 255:
        assert 0 < want["result"][3] < n


def test_more_ops_than_one_round_of_any_grid():
    """One op more than a full pass of the widest launch (the length kernel's grid cap x 256 lanes; the write
    kernels take 2 x 16 and 2 x 4 records per block and round): every grid-stride loop goes round again."""
    n = max(GRID_CAP * 256, 2 * COPY_GRID_CAP * 256 // 16, 2 * COPY_GRID_CAP * 256 // 64) + 1
    want = check(_tiny_ops(n, 5))
    assert want["result"][0] == n and all(2 <= len(r) <= 8 for r in want["records"][:1000])


# ---- varint boundaries -----------------------------------------------------------------------------------

BOUNDARY = (0, 1, 127, 128, 16383, 16384)


def test_key_and_value_lengths_at_the_varint_boundaries():
    rng = random.Random(3)
    ops = [EM.put(rng.randbytes(a), rng.randbytes(b)) for a in BOUNDARY for b in BOUNDARY]
    ops += [EM.delete(rng.randbytes(a), rng.randbytes(a % 5)) for a in BOUNDARY]
    want = check(ops)
    assert want["result"][L.RIO_WALENC_R_MAX_KEY_LEN] == 16384 and want["records"][0] == b"\x0a\x00"


def test_values_around_two_to_the_21():
    rng = random.Random(4)
    check([EM.put(b"below", rng.randbytes((1 << 21) - 1)), EM.delete(b"between"), EM.put(b"at", rng.randbytes(1 << 21))])


def test_body_lengths_at_the_varint_boundaries():
    rng = random.Random(5)
    ops = []
    for body in (127, 128, 16383, 16384, (1 << 21) - 1, 1 << 21):
        rest = body - 18  # a 16-byte key's field takes 18 bytes
        vlen = next(v for v in range(rest - 5, rest) if EM.field_len(v) == rest)
        ops.append(EM.put(rng.randbytes(16), rng.randbytes(vlen)))
        assert EM.body_len(ops[-1]) == body
    ops += [EM.delete(rng.randbytes(125)), EM.delete(rng.randbytes(126)), EM.delete(rng.randbytes(16381)), EM.delete(rng.randbytes(16382))]
    assert [EM.body_len(o) for o in ops[-4:]] == [127, 128, 16384, 16385]
    ops.append(EM.delete(rng.randbytes(16380)))
    assert EM.body_len(ops[-1]) == 16383
    check(ops)


# ---- copy edges ------------------------------------------------------------------------------------------

EDGE_LENGTHS = list(range(49)) + [LONG_ITEM - 1, LONG_ITEM, LONG_ITEM + 1]


@pytest.mark.parametrize("target", ["key", "value"])
def test_every_length_at_every_source_and_destination_alignment(target):
    """The probed item (an upsert's key next to a 3-byte value, or its value next to a 5-byte key: so a long key
    stands beside a short value and a long value beside a short key, and each instantiation writes headers) of
    every edge length at every (source mod 16, destination mod 16): a padding upsert before each probe moves the
    source by its own item of that arena and the destination by its record's length."""
    rng = random.Random(16)
    ops, reached = [], {n: set() for n in EDGE_LENGTHS if n}
    K = V = Rpos = 0  # the arenas' lengths so far
    for n in EDGE_LENGTHS:
        for a in range(16 if n else 1):
            for b in range(16 if n else 1):
                probe = EM.put(rng.randbytes(n), b"val") if target == "key" else EM.put(b"a key", rng.randbytes(n))
                rec = EM.record(probe)
                # the item's first byte inside its record
                inside = len(rec) - n if target == "value" else 1 + len(P.put_varint(EM.body_len(probe))) + 1 + len(P.put_varint(n))
                assert rec[inside:inside + n] == (probe[1] if target == "value" else probe[0])
                p = (a - (K if target == "key" else V)) % 16  # the pad's item in the probed arena
                for q in range(20):  # the pad's other item sets the destination
                    pad = EM.put(b"p" * p, b"q" * q) if target == "key" else EM.put(b"q" * q, b"p" * p)
                    if (Rpos + len(EM.record(pad)) + inside) % 16 == b or not n:
                        break
                else:
                    raise AssertionError("no pad reaches the destination")
                for op in (pad, probe):
                    ops.append(op)
                    K, V, Rpos = K + len(op[0]), V + len(op[1]), Rpos + len(EM.record(op))
                if n:
                    src = (K - n if target == "key" else V - n) % 16
                    reached[n].add((src, (Rpos - len(rec) + inside) % 16))
    assert all(len(s) == 256 for s in reached.values())
    ops += [EM.delete(rng.randbytes(n), b"hidden") for n in EDGE_LENGTHS]  # a delete's long key writes its header too
    log = Log(ops)
    assert log.t["keys"].data_ptr() % 16 == 0 and log.t["values"].data_ptr() % 16 == 0
    want = check(ops, log)
    assert want["result"][L.RIO_WALENC_R_MAX_KEY_LEN] == (LONG_ITEM + 1)


# ---- deletes and empty items -----------------------------------------------------------------------------

def test_deletes_and_empty_items():
    rng = random.Random(6)
    ops = [EM.delete(b"key", b"a value range behind the nil flag"), EM.delete(b"", b"hidden"), EM.delete(b""), EM.put(b"", b""),
           EM.put(b"k", b""), EM.put(b"", b"v"), EM.delete(rng.randbytes(LONG_ITEM + 7), rng.randbytes(LONG_ITEM + 9)),
           EM.put(rng.randbytes(LONG_ITEM), b""), EM.put(b"", rng.randbytes(LONG_ITEM)), EM.delete(b"last", b"x" * 50)]
    want = check(ops)
    assert want["records"][:4] == [b"\x12\x05\x12\x03key", b"\x12\x00", b"\x12\x00", b"\x0a\x00"]
    assert want["result"][2:4] == [5, 5] and b"hidden" not in want["arena"]
    check(EM.corpus(7, 3000))


# ---- capacity and bad input ------------------------------------------------------------------------------

@pytest.mark.parametrize("last", [EM.put(b"a short last key", b"and its value"), EM.put(b"k" * 40, bytes(range(256)) * 5),
                                  EM.put(b"K" * (LONG_ITEM + 3), b"v"), EM.delete(b"the last key")],
                         ids=["short", "long value", "long key", "delete"])
def test_records_cap_exact_and_one_byte_short(last):
    ops = EM.corpus(8, 400) + [last]
    want = EM.expected(ops)
    total, fill = want["rec_off"][-1], bytes([FILL])
    log = Log(ops)
    rec_off, res, arena = encode(log, total)
    assert (rec_off, res) == (want["rec_off"], want["result"])
    assert arena == want["arena"] + fill * CANARY
    # one byte short: the last record would pass the cap and is not written, everything before it is, and the
    # offsets and the result are complete
    rec_off, res, arena = encode(log, total - 1)
    assert (rec_off, res) == (want["rec_off"], want["result"])
    kept = want["rec_off"][-2]
    assert arena == want["arena"][:kept] + fill * (total - 1 - kept + CANARY)
    # no capacity at all: offsets and result only
    out = Out(log.n, 0)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        rc = L.lib().rio_wal_ops_encode(ctx(), ctypes.addressof(log.view), None, 0, out.rec_off.data_ptr(), out.res.data_ptr(),
                                        ctypes.c_void_p(st.cuda_stream))
    st.synchronize()
    assert rc == L.RIO_OK and out.read()[:2] == (want["rec_off"], want["result"])


def _bad(log_arrays, key_bytes=None, value_bytes=None):
    log = Log(arrays=log_arrays, key_bytes=key_bytes, value_bytes=value_bytes)
    _, res, arena = encode(log)
    assert arena[log.bound():] == bytes([FILL]) * CANARY
    want = EM.first_bad(log_arrays[1], log_arrays[3], log.key_bytes, log.value_bytes)
    assert res[L.RIO_WALENC_R_FIRST_BAD] == want
    assert res[L.RIO_WALENC_R_BAD_CLASS] == (EM.RANGE if want != _NONE else 0)
    return want


def test_bad_ranges_in_different_blocks_report_the_smaller_op():
    """Ops 10 and 499 / 500 are handled by different workgroups (256 lanes each)."""
    ops = EM.corpus(9, 600)
    keys, key_off, values, val_off, flags = EM.arrays(ops)
    assert key_off[10] > 0 and _bad((keys, key_off, values, val_off, flags)) == _NONE
    ko, vo = key_off.copy(), val_off.copy()
    ko[11] = ko[10] - 1                 # op 10's key runs backwards
    vo[500] = len(values) + 1000        # op 499's value leaves its arena, op 500's starts outside it
    assert _bad((keys, ko, values, vo, flags)) == 10
    assert _bad((keys, key_off, values, vo, flags)) == 499
    # the other way round: the range that leaves its arena first, the one that is not monotone behind it
    ko, vo = key_off.copy(), val_off.copy()
    ko[10] = len(keys) + (1 << 40)      # far outside: op 9 ends there, op 10 starts there
    vo[501] = vo[500] - 1
    assert _bad((keys, ko, values, vo, flags)) == 9
    assert _bad((keys, key_off, values, vo, flags)) == 500
    # arena lengths shorter than the offsets: the first op that leaves them
    cut = int(key_off[300]) + 1
    first = next(i for i in range(600) if key_off[i + 1] > cut)
    assert _bad((keys, key_off, values, val_off, flags), key_bytes=cut) == first > 256
    cut = int(val_off[120]) + 1
    first = next(i for i in range(600) if val_off[i + 1] > cut)
    assert _bad((keys, key_off, values, val_off, flags), value_bytes=cut) == first
    # a delete's value range is checked as every range is, though its bytes are not read
    d = next(i for i in range(300, 600) if ops[i][2])
    vo = val_off.copy()
    vo[d + 1:] += 1 << 33
    assert _bad((keys, key_off, values, vo, flags)) == d
    check(ops)


# ---- streams and graphs ----------------------------------------------------------------------------------

def test_the_context_stream_and_a_callers_stream_agree():
    ops = EM.corpus(10, 700)
    want = EM.expected(ops)
    log = Log(ops)
    out = Out(log.n, log.bound())
    torch.cuda.synchronize()
    out.launch(log, None)  # the context's own stream
    torch.cuda.synchronize()
    rec_off, res, arena = out.read()
    assert (rec_off, res) == (want["rec_off"], want["result"]) and arena[:rec_off[-1]] == want["arena"]
    assert encode(log) == (rec_off, res, arena)


def test_capture_in_a_graph_and_replay_with_other_bytes():
    ops = EM.corpus(11, 2000) + [EM.put(b"k" * 30, bytes(LONG_ITEM + 11)), EM.delete(b"d" * (LONG_ITEM + 1))]
    log = Log(ops)
    out = Out(log.n, log.bound())
    s = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    st = ctypes.c_void_p(s.cuda_stream)
    out.launch(log, st)  # one call first: the context's scratch is sized for this n, the capture allocates nothing
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out.launch(log, st)
    rng = random.Random(12)
    for _ in range(2):
        # the same n and arena lengths, other bytes and other lengths per op: the ops in another order
        rng.shuffle(ops)
        other = Log(ops)
        for name, t in log.t.items():
            t.copy_(other.t[name])
        out.records.fill_(FILL)
        out.rec_off.fill_(-1)
        out.res.fill_(-1)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        want = EM.expected(ops)
        rec_off, res, arena = out.read()
        assert (rec_off, res) == (want["rec_off"], want["result"])
        assert arena == want["arena"] + bytes([FILL]) * (log.bound() + CANARY - rec_off[-1])


# ---- round trip on the device ----------------------------------------------------------------------------

def test_encoded_records_parse_back_to_the_ops():
    ops = EM.accepted_corpus(13, 3000) + [EM.put(b"long", random.Random(1).randbytes(3 * LONG_ITEM))]
    keys, key_off, values, val_off, flags = EM.arrays(ops)
    log = Log(ops)
    out = Out(log.n, log.bound())
    n = log.n
    zero = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
    res = torch.empty(L.RIO_WAL_RESULT_WORDS, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    lib = L.lib()
    with torch.cuda.stream(st):
        h = ctypes.c_void_p(st.cuda_stream)
        out.launch(log, h)
        total = int(out.rec_off[n].item())
        seg = (L.WalSegment * 1)(L.WalSegment(out=out.records.data_ptr(), out_off=out.rec_off.data_ptr(), flags=zero.data_ptr(),
                                              n=n, out_bytes=total))
        assert lib.rio_wal_ops_plan(ctx(), ctypes.addressof(seg), 1, res.data_ptr(), h) == L.RIO_OK
        r = [x & _NONE for x in res.cpu().tolist()]
        assert r == [n, n, len(keys), len(values), max(len(o[0]) for o in ops), _NONE, 0, 0]
        back = dict(keys=torch.empty(len(keys) + 1, dtype=torch.uint8, device="cuda"),
                    values=torch.empty(len(values) + 1, dtype=torch.uint8, device="cuda"),
                    key_off=torch.empty(n + 1, dtype=torch.int64, device="cuda"),
                    val_off=torch.empty(n + 1, dtype=torch.int64, device="cuda"), flags=torch.empty(n, dtype=torch.uint8, device="cuda"))
        assert lib.rio_wal_ops_gather(ctx(), n, back["keys"].data_ptr(), len(keys), back["key_off"].data_ptr(),
                                      back["values"].data_ptr(), len(values), back["val_off"].data_ptr(),
                                      back["flags"].data_ptr(), None, h) == L.RIO_OK
    st.synchronize()
    assert back["keys"][:len(keys)].cpu().numpy().tobytes() == keys and back["values"][:len(values)].cpu().numpy().tobytes() == values
    assert back["key_off"].cpu().tolist() == key_off.tolist() and back["val_off"].cpu().tolist() == val_off.tolist()
    assert back["flags"].cpu().tolist() == flags.tolist()


# ---- end to end ------------------------------------------------------------------------------------------

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


def _batch(ops):
    b = DB.WriteBatch()
    for key, value, nil in ops:
        assert (b.DeleteBytes(key) if nil else b.PutBytes(key, value)) is None
    assert len(b) == len(ops)
    return b


@pytest.fixture(scope="module")
def workload():
    return EM.accepted_corpus(21, 4000, keys=600)


@pytest.mark.parametrize("comp", [L.COMP_NONE, L.COMP_SNAPPY], ids=["none", "snappy"])
@pytest.mark.parametrize("earlier", [0, 150], ids=["fresh", "after appends"])
def test_append_batch_writes_the_host_loops_directory(tmp_path, workload, comp, earlier):
    before, ops = workload[:earlier], workload[earlier:]
    max_size = 64 << 10
    want_dir, got_dir, table = str(tmp_path / "want"), str(tmp_path / "got"), str(tmp_path / "table")
    want, got = _appender(want_dir, comp, max_size), _appender(got_dir, comp, max_size)
    for op in before + ops:
        assert want.Append(EM.record(op)) is None
    assert want.Close() is None
    for op in before:
        assert got.Append(EM.record(op)) is None
    dev_ops, err = DB.append_batch(got, _batch(ops))
    assert err is None, err
    assert got.nextWriterNumber == want.nextWriterNumber
    assert got.Close() is None
    a, b = _snapshot(want_dir), _snapshot(got_dir)
    assert len(a) >= 3 and list(a) == list(b)
    assert a == b
    if earlier:
        return
    # the same device arrays flush to the table recovery writes from the directory
    assert dev_ops.view.n == len(ops) and dev_ops.max_key_len == 9
    with torch.cuda.device(0):
        c = MS.flush_ops_on_device(ctx(), 0, dev_ops.view, L.RIO_FLUSH_WITH_TOMBSTONES, L.COMP_SNAPPY,
                                   max_key_len=dev_ops.max_key_len)
        assert c.status is None
        ends = [int(x) & _NONE for x in c.out_src[[0, c.n_out - 1]].cpu().tolist()]
        lo, hi = (ops[e][0] for e in ends)
        flushed = str(tmp_path / "flushed")
        from sstables.merger import write_table_files

        write_table_files(flushed, c, lo, hi)
        torch.cuda.synchronize()
    n, wrote, err = DB.recover_wal(got_dir, table)
    assert err is None, err
    assert (n, wrote) == (len(ops), True)
    for name in FM.FILES:
        assert open(os.path.join(table, name), "rb").read() == open(os.path.join(flushed, name), "rb").read(), name


def test_append_batch_of_a_device_log_and_refusals(tmp_path, workload):
    ops = workload[:500]
    want, got = _appender(str(tmp_path / "want"), L.COMP_SNAPPY, 1 << 20), _appender(str(tmp_path / "got"), L.COMP_SNAPPY, 1 << 20)
    for op in ops:
        assert want.Append(EM.record(op)) is None
    assert want.Close() is None
    log = Log(ops)
    torch.cuda.synchronize()
    holder, err = DB.append_batch(got, log.view)  # a log that is on the device already
    assert err is None and holder.view is log.view
    _, err = DB.append_batch(got, DB.WriteBatch())  # nothing to append
    assert err is None and got.Close() is None
    assert _snapshot(str(tmp_path / "want")) == _snapshot(str(tmp_path / "got"))
    gz = _appender(str(tmp_path / "gz"), L.COMP_GZIP, 1 << 20)
    import sstables as S

    assert isinstance(DB.append_batch(gz, _batch(ops))[1], S.UnsupportedError)
    # an inconsistent log is refused with its first bad op, and nothing is written
    keys, key_off, values, val_off, flags = EM.arrays(ops)
    key_off = key_off.copy()
    key_off[41] = key_off[40] - 1
    bad = Log(arrays=(keys, key_off, values, val_off, flags))
    fresh = _appender(str(tmp_path / "fresh"), L.COMP_NONE, 1 << 20)
    torch.cuda.synchronize()
    _, err = DB.append_batch(fresh, bad.view)
    assert err is not None and "op 40 " in str(err) and fresh.currentWriter.Size() == 8
