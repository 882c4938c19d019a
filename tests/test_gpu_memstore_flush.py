"""Memstore flush on the device (GPU): MemStore.Flush / FlushWithTombstones and the lower-level
flush_ops_on_device against flush_model (ops applied to a dict, sorted) written out by the host writer. For
every case and both modes the three output files must be byte-identical to the model's table; the device
output is then reopened with NewSSTableReader (validation on) and its scan compared with the model's pairs."""
import ctypes
import os
import random
import re
import struct

import numpy as np
import pytest
import torch

import compact_model as CM
import flush_model as FM
import memstore as MS
import sstables as S
from conftest import PKG
from recordio import _lib as L
from sstables.merger import write_table_files
from sstables.writer import write_sstable
from test_gpu_compact import _ordering_tables, scan_all

pytestmark = pytest.mark.gpu

MODES = (FM.WITH_TOMBSTONES, FM.SKIP_TOMBSTONES)
_NONE = 0xFFFFFFFFFFFFFFFF


def be(i):
    return struct.pack(">I", i)


def same_files(got, want):
    for name in FM.FILES:
        a, b = open(os.path.join(got, name), "rb").read(), open(os.path.join(want, name), "rb").read()
        assert len(a) == len(b), (name, len(a), len(b))
        assert a == b, name


def reopen(got, pairs, meta):
    r, err = S.NewSSTableReader(S.ReadBasePath(got))
    assert err is None, err
    assert scan_all(r) == pairs
    md = r.MetaData()
    assert md.numRecords == len(pairs) == meta.numRecords
    assert md.nullValues == sum(v is None for _, v in pairs) == meta.nullValues
    return r


def check(tmp_path, ops, comp=None):
    """The ops through a MemStore's public calls, flushed in both modes."""
    m = FM.fill(MS.NewMemStore(), ops)
    out = {}
    for mode in MODES:
        want, got = str(tmp_path / f"want{mode}"), str(tmp_path / f"got{mode}")
        pairs, meta = FM.write_expected(want, ops, mode, 2 if comp is None else comp)
        opts = [S.WriteBasePath(got)] + ([] if comp is None else [S.DataCompressionType(comp)])
        err = (m.Flush if mode == FM.SKIP_TOMBSTONES else m.FlushWithTombstones)(*opts)
        assert err is None, err
        same_files(got, want)
        reopen(got, pairs, meta)
        out[mode] = pairs
    return out


class DeviceLog:
    """An op log in device memory as rio_ops_view takes it (arrays given as numpy, or built from ops)."""

    def __init__(self, keys, key_off, values, val_off, flags):
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()  # noqa: E731
        pad = np.zeros(L.RIO_DEVICE_PAD, dtype=np.uint8)
        self.h_keys, self.h_key_off = np.asarray(keys, dtype=np.uint8), np.asarray(key_off, dtype=np.int64)
        self.n = len(flags)
        self.t = [up(np.concatenate([self.h_keys, pad]), np.uint8), up(key_off, np.int64),
                  up(np.concatenate([np.asarray(values, dtype=np.uint8), pad]), np.uint8), up(val_off, np.int64),
                  up(np.concatenate([np.asarray(flags, dtype=np.uint8), pad[:1]]), np.uint8)]
        self.view = L.OpsView(keys=self.t[0].data_ptr(), key_off=self.t[1].data_ptr(), values=self.t[2].data_ptr(),
                              val_off=self.t[3].data_ptr(), flags=self.t[4].data_ptr(), n=self.n, key_bytes=len(keys),
                              value_bytes=len(values))

    @classmethod
    def of(cls, ops):
        keys = b"".join(k for k, _ in ops)
        values = b"".join(v or b"" for _, v in ops)
        key_off = np.cumsum([0] + [len(k) for k, _ in ops])
        val_off = np.cumsum([0] + [len(v or b"") for _, v in ops])
        return cls(np.frombuffer(keys, dtype=np.uint8), key_off, np.frombuffer(values, dtype=np.uint8), val_off,
                   [L.RIO_FLAG_NIL if v is None else 0 for _, v in ops])

    def key(self, op):
        return self.h_keys[self.h_key_off[op]:self.h_key_off[op + 1]].tobytes()

    def flush(self, path, mode, max_key_len, comp=L.COMP_SNAPPY):
        c = MS.flush_ops_on_device(L.default_ctx(0), 0, self.view, mode, comp, max_key_len=max_key_len)
        if c.status is None:
            lo = hi = b""
            if c.n_out:
                first, last = (int(x) & _NONE for x in c.out_src[[0, c.n_out - 1]].cpu().tolist())
                lo, hi = self.key(first), self.key(last)
            write_table_files(path, c, lo, hi)
        return c


def check_log(tmp_path, ops, max_key_len, log=None):
    """The ops as a device-resident log through flush_ops_on_device, with the key bound given."""
    log = log or DeviceLog.of(ops)
    for mode in MODES:
        want, got = str(tmp_path / f"lwant{mode}"), str(tmp_path / f"lgot{mode}")
        pairs, meta = FM.write_expected(want, ops, mode)
        c = log.flush(got, mode, max_key_len)
        assert c.status is None and c.first_dup == _NONE and c.n_out == len(pairs)
        same_files(got, want)
        reopen(got, pairs, meta)


# ---- the reference's flush tests (memstore_test.go:165-292), through Get -------------------------------

def _ref_store():
    m = MS.NewMemStore()
    assert m.Upsert(b"akey", b"aval") is None and m.Upsert(b"bkey", b"bval") is None
    return m


def test_reference_flush(tmp_path):  # TestMemStoreFlush
    base = str(tmp_path / "t")
    assert _ref_store().Flush(S.WriteBasePath(base)) is None
    r, err = S.NewSSTableReader(S.ReadBasePath(base), S.ReadWithKeyComparator())
    assert err is None, err
    assert r.Get(b"akey") == (b"aval", None) and r.Get(b"bkey") == (b"bval", None)
    assert r.Get(b"ckey") == (None, S.NotFound)
    assert r.Close() is None


def test_reference_flush_ignores_tombstones(tmp_path):  # TestMemStoreFlushTombStonesIgnore
    m, base = _ref_store(), str(tmp_path / "t")
    assert m.Delete(b"akey") is None
    assert m.Flush(S.WriteBasePath(base)) is None
    r, err = S.NewSSTableReader(S.ReadBasePath(base))
    assert err is None, err
    assert r.Get(b"akey") == (None, S.NotFound)
    assert r.Get(b"bkey") == (b"bval", None) and r.Get(b"ckey") == (None, S.NotFound)


def test_reference_flush_with_tombstones(tmp_path):  # TestMemStoreFlushWithTombStonesInclusive
    m, base = _ref_store(), str(tmp_path / "t")
    assert m.Delete(b"akey") is None
    assert m.FlushWithTombstones(S.WriteBasePath(base)) is None
    r, err = S.NewSSTableReader(S.ReadBasePath(base))
    assert err is None, err
    assert r.Get(b"akey") == (None, None)  # found, nil
    assert r.Get(b"bkey") == (b"bval", None) and r.Get(b"ckey") == (None, S.NotFound)


def test_reference_tombstone_behavior(tmp_path):  # TestMemStoreTombstoneBehavior
    m, base = MS.NewMemStore(), str(tmp_path / "t")
    assert m.Upsert(b"akey", b"aval") is None and m.Tombstone(b"akey") is None and m.Tombstone(b"bkey") is None
    assert m.FlushWithTombstones(S.WriteBasePath(base)) is None
    r, err = S.NewSSTableReader(S.ReadBasePath(base))
    assert err is None, err
    assert r.Get(b"akey") == (None, None) and r.Get(b"bkey") == (None, None)
    assert r.MetaData().numRecords == 2 and r.MetaData().nullValues == 2


# ---- sizes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257])
def test_distinct_key_counts(tmp_path, n):
    """Around a wave and a block of lanes; every third key is rewritten, every fifth ends tombstoned."""
    rng = random.Random(n)
    ops = [(be(i * 2654435761 & 0xFFFFFFFF), b"v%d" % i) for i in range(n)]
    ops += [(k, b"again" + k) for k, _ in ops[::3]] + [(k, None) for k, _ in ops[::5]]
    rng.shuffle(ops)
    out = check(tmp_path, ops)
    assert len(out[FM.WITH_TOMBSTONES]) == n


def test_more_ops_than_one_round_of_the_grid(tmp_path):
    """540 000 ops on 5 000 keys: more than the launch helper's largest grid x block, so every grid-stride loop
    of rio_flush.hip goes round again (and the sort runs at a size past its small-input paths)."""
    cap = int(re.search(r"kFlushGridCap = (\d+);", open(os.path.join(PKG, "csrc", "rio_flush.hip")).read()).group(1))
    n = 540_000
    assert n > cap * 256
    rng = np.random.default_rng(11)
    ids = rng.integers(0, 5000, n).astype(">u4")
    nil = rng.random(n) < 0.1
    vals = (np.arange(n) % 65521).astype("<u2")
    val_len = np.where(nil, 0, 2)
    val_off = np.concatenate([[0], np.cumsum(val_len)])
    values = vals[~nil].view(np.uint8)
    log = DeviceLog(ids.view(np.uint8), np.arange(n + 1) * 4, values, val_off, nil.astype(np.uint8) * L.RIO_FLAG_NIL)
    kb, vb = ids.tobytes(), vals.tobytes()
    ops = [(kb[4 * i:4 * i + 4], None if nil[i] else vb[2 * i:2 * i + 2]) for i in range(n)]
    check_log(tmp_path, ops, 4, log)


# ---- key shapes ----------------------------------------------------------------------------------------

def _ordering_ops():
    """test_gpu_compact's ordering set (a, a\\0, a\\0\\0, bytes >= 0x80, the 8/9/16/17-byte boundaries, lengths
    1 .. 40) as ops, table after table, so a key of several tables is rewritten; plus the empty key."""
    ops = [(k, v) for t in _ordering_tables() for k, v in t]
    random.Random(3).shuffle(ops)
    return ops[:40] + [(b"", b"the empty key")] + ops[40:] + [(ops[7][0], None), (b"", b"")]


def test_key_ordering_prefixes_and_high_bytes(tmp_path):
    ops = _ordering_ops()
    out = check(tmp_path, ops)
    assert [k for k, _ in out[FM.WITH_TOMBSTONES]] == sorted({k for k, _ in ops})
    assert out[FM.SKIP_TOMBSTONES][0] == (b"", b"")


def test_keys_sharing_a_24_byte_prefix(tmp_path):
    p = b"twenty-four bytes prefix!"[:24]
    rng = random.Random(24)
    ops = [(p + rng.randbytes(rng.randint(0, 12)), b"v%d" % i) for i in range(700)]
    ops += [(p, b"the prefix itself"), (p[:23], b"shorter"), (p + b"\0", None)]
    rng.shuffle(ops)
    check(tmp_path, ops)


def test_keys_equal_but_for_trailing_zeros(tmp_path):
    """Equal in every zero-padded chunk: only the length pass tells them apart, across the chunk boundary."""
    ops = []
    for stem in (b"", b"abcde", b"abcdefg", b"abcdefgh", b"abcdefghijklmno", b"abcdefghijklmnop"):
        ops += [(stem + bytes(j), b"%d zeros after %d" % (j, len(stem))) for j in range(0, 19)]
    random.Random(8).shuffle(ops)
    ops += [(k, b"second " + v) for k, v in ops[::4]]
    out = check(tmp_path, ops)
    assert [k for k, _ in out[FM.SKIP_TOMBSTONES]] == sorted({k for k, _ in ops})


def test_keys_of_the_longest_supported_length(tmp_path):
    """Keys of exactly max_key_len = RIO_FLUSH_MAX_KEY_LEN (129 passes), differing in the first, a middle and
    the last byte, next to short ones."""
    n = L.RIO_FLUSH_MAX_KEY_LEN
    base = bytes(range(256)) * (n // 256)
    ops = [(base, b"base"), (base[:-1] + b"\x00", b"last byte"), (b"\xfe" + base[1:], b"first byte"),
           (base[:500] + b"\xff" + base[501:], b"middle"), (base[:n - 1], b"one shorter"), (b"z", b"short"),
           (base, b"base again"), (base[:8], None)]
    check(tmp_path, ops)


@pytest.mark.parametrize("bound", [41, 48, 200])
def test_key_bound_larger_than_any_key(tmp_path, bound):
    ops = _ordering_ops()
    assert max(len(k) for k, _ in ops) == 41
    check_log(tmp_path, ops, bound)


# ---- latest wins ---------------------------------------------------------------------------------------

def test_one_key_with_a_thousand_interleaved_ops(tmp_path):
    rng = random.Random(1000)
    ops = []
    for i in range(1000):
        ops.append((b"the hot key", None if i % 7 == 3 else b"hot %d" % i))
        ops.append((b"other %d" % rng.randrange(50), b"o%d" % i))
    out = check(tmp_path, ops)
    assert (b"the hot key", b"hot 999") in out[FM.SKIP_TOMBSTONES]


def test_sequences_on_one_key(tmp_path):
    seqs = {b"upsert delete upsert": [b"1", None, b"3"], b"upsert delete": [b"1", None],
            b"tombstone upsert": [None, b"2"], b"latest empty": [b"full", b""], b"empty then nil": [b"", None],
            b"nil nil": [None, None], b"three upserts": [b"a", b"bb", b"ccc"]}
    ops = []
    for step in range(3):  # the sequences advance together, so each key's ops are apart in the log
        ops += [(k, vs[step]) for k, vs in seqs.items() if step < len(vs)]
    out = check(tmp_path, ops)
    assert out[FM.SKIP_TOMBSTONES] == sorted([(b"upsert delete upsert", b"3"), (b"tombstone upsert", b"2"),
                                              (b"latest empty", b""), (b"three upserts", b"ccc")])
    assert dict(out[FM.WITH_TOMBSTONES])[b"upsert delete"] is None


def test_all_ops_on_one_key(tmp_path):
    out = check(tmp_path / "set", [(b"k", b"%d" % i) for i in range(300)])
    assert out[FM.SKIP_TOMBSTONES] == [(b"k", b"299")]
    out = check(tmp_path / "gone", [(b"k", b"%d" % i) for i in range(300)] + [(b"k", None)])
    assert out[FM.SKIP_TOMBSTONES] == [] and out[FM.WITH_TOMBSTONES] == [(b"k", None)]


def test_all_keys_tombstoned(tmp_path):
    n = 130
    ops = [(be(i), b"v") for i in range(n)] + [(be(i), None) for i in reversed(range(n))]
    out = check(tmp_path, ops)  # check() compares nullValues of both tables with the pairs
    assert out[FM.SKIP_TOMBSTONES] == [] and out[FM.WITH_TOMBSTONES] == [(be(i), None) for i in range(n)]
    m, _ = S.proto.read_metadata_if_exists(str(tmp_path / f"got{FM.WITH_TOMBSTONES}" / "meta.pb.bin"))
    assert m.numRecords == n and m.nullValues == n
    m, _ = S.proto.read_metadata_if_exists(str(tmp_path / f"got{FM.SKIP_TOMBSTONES}" / "meta.pb.bin"))
    assert m.numRecords == 0 and m.nullValues == 0 and m.minKey == b"" and m.maxKey == b""


def test_arrival_order_does_not_change_the_files(tmp_path):
    rng = random.Random(77)
    keys = sorted({rng.randbytes(rng.randint(1, 20)) for _ in range(900)})
    val = lambda k: None if k[0] % 9 == 0 else b"value of " + k  # noqa: E731
    orders = {"asc": keys, "desc": keys[::-1], "rand": rng.sample(keys, len(keys))}
    for name, order in orders.items():
        check(tmp_path / name, [(k, val(k)) for k in order])
    for mode in MODES:
        for name in FM.FILES:
            a, d, r = (open(str(tmp_path / o / f"got{mode}" / name), "rb").read() for o in orders)
            assert a == d == r, (mode, name)


# ---- values and output compression ---------------------------------------------------------------------

@pytest.mark.parametrize("comp", [L.COMP_NONE, L.COMP_SNAPPY])
def test_value_lengths_both_gather_paths(tmp_path, comp):
    """0, 1, 15 / 16 / 17 and 1023 / 1024 / 1025 bytes (the lane-group and the wave copy), as winners and as
    overwritten losers, half random and half compressible."""
    rng = random.Random(5)
    val = lambda n: rng.randbytes(n // 2) + bytes(n - n // 2)  # noqa: E731
    lens = (0, 1, 15, 16, 17, 1023, 1024, 1025)
    ops = [(b"key %02d" % j, val(n)) for j, n in enumerate(lens)]
    ops += [(b"key %02d" % j, val(lens[(j + 3) % len(lens)])) for j in range(0, len(lens), 2)]
    ops += [(b"odd %d" % j, val(3 + 2 * j)) for j in range(6)]
    check(tmp_path, ops, comp)


# ---- the flushed table as a compaction input -----------------------------------------------------------

def test_flushed_table_merges_with_a_host_written_one(tmp_path):
    rng = random.Random(21)
    ops = [(be(rng.randrange(400)), None if rng.random() < 0.2 else b"mem %d" % i) for i in range(1500)]
    m, flushed = FM.fill(MS.NewMemStore(), ops), str(tmp_path / "flushed")
    assert m.FlushWithTombstones(S.WriteBasePath(flushed)) is None
    older = [(be(i), b"disk %d" % i) for i in range(0, 600, 2)]
    write_sstable(str(tmp_path / "older"), older)
    readers = []
    for base in ("older", "flushed"):
        r, err = S.NewSSTableReader(S.ReadBasePath(str(tmp_path / base)))
        assert err is None, err
        readers.append(r)
    tables = [older, FM.flush_pairs(ops, FM.WITH_TOMBSTONES)]
    for name, reduce, model in (("latest", S.ScanReduceLatestWins, CM.reduce_latest_wins),
                                ("skip", S.ScanReduceLatestWinsSkipTombstones, CM.reduce_latest_wins_skip_tombstones)):
        got, want = str(tmp_path / f"got_{name}"), str(tmp_path / f"want_{name}")
        assert S.NewSSTableMerger().MergeCompact(readers, got, reduce) is None
        write_sstable(want, CM.merge_compact(tables, model))
        same_files(got, want)


# ---- rejected input at the C level ---------------------------------------------------------------------

def _plan_result(view, mode, max_key_len):
    n = int(view.n)
    src = torch.empty(n, dtype=torch.int64, device="cuda")
    keep = torch.empty(n, dtype=torch.uint8, device="cuda")
    res = torch.empty(L.RIO_MERGE_RESULT_WORDS, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        rc = L.lib().rio_sst_flush_plan(L.default_ctx(0), ctypes.addressof(view), mode, max_key_len, src.data_ptr(),
                                        keep.data_ptr(), res.data_ptr(), ctypes.c_void_p(st.cuda_stream))
        assert rc == L.RIO_OK
    st.synchronize()
    return [x & _NONE for x in res.cpu().tolist()]


@pytest.mark.parametrize("mode", MODES)
def test_inconsistent_log_is_reported_by_op(tmp_path, mode):
    """A key longer than max_key_len and a val_off that leaves the arena: the plan reports the op in
    RIO_MERGE_R_UNSORTED (every index stays clamped), flush_ops_on_device stops there, nothing is written."""
    ops = [(b"key%03d" % i, b"value %d" % i) for i in range(300)]
    ops[123] = (b"a key that is longer", b"x")
    log = DeviceLog.of(ops)
    r = _plan_result(log.view, mode, 6)
    assert r[L.RIO_MERGE_R_UNSORTED] == 123 and r[L.RIO_MERGE_R_FIRST_DUP] == _NONE
    assert _plan_result(log.view, mode, 20)[L.RIO_MERGE_R_UNSORTED] == _NONE
    c = log.flush(str(tmp_path / "long"), mode, 6)
    assert c.status == "unsorted" and c.unsorted_table == 123 and c.out_src is None

    ops = [(b"key%03d" % i, b"value %d" % i) for i in range(300)]
    good = DeviceLog.of(ops)
    val_off = good.t[3].cpu().numpy().copy()
    val_off[201] = val_off[-1] + (1 << 40)  # op 200's value ends far outside the arena
    bad = DeviceLog(good.h_keys, good.h_key_off, good.t[2].cpu().numpy()[:val_off[-1]], val_off,
                    np.zeros(300, dtype=np.uint8))
    bad.view.value_bytes = int(good.view.value_bytes)
    assert _plan_result(bad.view, mode, 6)[L.RIO_MERGE_R_UNSORTED] == 200
    c = bad.flush(str(tmp_path / "off"), mode, 6)
    assert c.status == "unsorted" and c.unsorted_table == 200
    key_off = good.h_key_off.copy()
    key_off[50] = key_off[49] - 1  # op 49's key range runs backwards
    bad = DeviceLog(good.h_keys, key_off, good.t[2].cpu().numpy()[:val_off[-1]], good.t[3].cpu().numpy(),
                    np.zeros(300, dtype=np.uint8))
    assert _plan_result(bad.view, mode, 6)[L.RIO_MERGE_R_UNSORTED] == 49
    assert not os.path.exists(str(tmp_path / "long")) and not os.path.exists(str(tmp_path / "off"))


# ---- stage timing --------------------------------------------------------------------------------------

def test_stage_times_of_the_last_plan(tmp_path):
    """rio_sst_flush_stage_ms: check, the length pass, one pass per 8-byte chunk, keep, crc while the
    context records stage events; nothing while it does not."""
    lib, ctx = L.lib(), L.default_ctx(0)
    log = DeviceLog.of([(b"key %05d" % (i * 7919 % 3000), b"v%d" % i) for i in range(5000)])  # 9-byte keys
    ms = (ctypes.c_float * 16)()
    assert lib.rio_ctx_set_timing(ctx, 1) == L.RIO_OK
    try:
        assert log.flush(str(tmp_path / "t"), FM.SKIP_TOMBSTONES, 9).n_out == 3000
        assert lib.rio_sst_flush_stage_ms(ctx, ms, 16) == 2 + 2 + 2
        assert all(0 <= x < 1000 for x in list(ms)[:6])
        assert lib.rio_sst_flush_stage_ms(ctx, ms, 2) == 2
    finally:
        assert lib.rio_ctx_set_timing(ctx, 0) == L.RIO_OK
    assert log.flush(str(tmp_path / "t"), FM.SKIP_TOMBSTONES, 9).n_out == 3000
    assert lib.rio_sst_flush_stage_ms(ctx, ms, 16) == 0
