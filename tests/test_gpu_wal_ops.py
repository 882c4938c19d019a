"""WAL recovery on the device (GPU): rio_wal_ops_plan / rio_wal_ops_gather against wal_model (every record through
the host mirror of proto.Unmarshal(WalMutation) and the switch of recovery.go:224-237), and simpledb.recover_wal end
to end against flush_model's table. Every case compares the device arrays (key_off, val_off, flags, op_rec, both
arenas) and the result block byte for byte with the model."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

import flush_model as FM
import gpu_util
import memstore as MS
import simpledb as DB
import sstables as S
import wal as W
import wal_model as WM
from conftest import PKG
from recordio import _lib as L
from simpledb import proto as P
from test_gpu_compact import scan_all
from wal_model import field, group, nested_groups

pytestmark = pytest.mark.gpu

_NONE = 0xFFFFFFFFFFFFFFFF
_SRC = open(os.path.join(PKG, "csrc", "rio_walops.hip")).read()
GRID_CAP = int(re.search(r"kWalGridCap = (\d+);", _SRC).group(1))
COPY_GRID_CAP = int(re.search(r"kWalCopyGridCap = (\d+);", _SRC).group(1))
LONG_ITEM = int(re.search(r"kWalLongItem = (\d+);", _SRC).group(1))
CANARY, FILL = 64, 0xA5


class Segment:
    """One decoded WAL file in device memory as rio_wal_segment takes it."""

    def __init__(self, records, out_off=None, out_bytes=None):
        arena = b"".join(r or b"" for r in records)
        off = np.cumsum([0] + [len(r or b"") for r in records]) if out_off is None else np.asarray(out_off)
        flags = [L.RIO_FLAG_NIL if r is None else 0 for r in records]
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()  # noqa: E731
        pad = np.zeros(L.RIO_DEVICE_PAD, dtype=np.uint8)
        self.t = [up(np.concatenate([np.frombuffer(arena, dtype=np.uint8), pad]), np.uint8), up(off, np.int64),
                  up(np.concatenate([np.asarray(flags, dtype=np.uint8), pad[:1]]), np.uint8)]
        self.c = L.WalSegment(out=self.t[0].data_ptr(), out_off=self.t[1].data_ptr(), flags=self.t[2].data_ptr(),
                              n=len(records), out_bytes=len(arena) if out_bytes is None else out_bytes)


def plan(segs):
    arr = (L.WalSegment * len(segs))(*[s.c for s in segs])
    res = torch.empty(L.RIO_WAL_RESULT_WORDS, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        rc = L.lib().rio_wal_ops_plan(L.default_ctx(0), ctypes.addressof(arr), len(segs), res.data_ptr(),
                                      ctypes.c_void_p(st.cuda_stream))
        assert rc == L.RIO_OK, rc
    st.synchronize()
    return [x & _NONE for x in res.cpu().tolist()]


def gather(n_ops, keys_cap, values_cap, with_op_rec=True):
    """-> key_off, val_off, flags, op_rec (lists), the key and value arenas with CANARY bytes past their caps."""
    filled = lambda n, dt: torch.full((max(n, 1),), FILL if dt == torch.uint8 else -1, dtype=dt, device="cuda")  # noqa: E731
    keys, values = filled(keys_cap + CANARY, torch.uint8), filled(values_cap + CANARY, torch.uint8)
    key_off, val_off = filled(n_ops + 1, torch.int64), filled(n_ops + 1, torch.int64)
    flags, op_rec = filled(n_ops + CANARY, torch.uint8), filled(n_ops, torch.int64)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        rc = L.lib().rio_wal_ops_gather(L.default_ctx(0), n_ops, keys.data_ptr(), keys_cap, key_off.data_ptr(),
                                        values.data_ptr(), values_cap, val_off.data_ptr(), flags.data_ptr(),
                                        op_rec.data_ptr() if with_op_rec else None, ctypes.c_void_p(st.cuda_stream))
        assert rc == L.RIO_OK, rc
    st.synchronize()
    assert (flags[n_ops:].cpu().numpy() == FILL).all()
    return dict(key_off=key_off.cpu().tolist(), val_off=val_off.cpu().tolist(), flags=flags[:n_ops].cpu().tolist(),
                op_rec=op_rec[:n_ops].cpu().tolist(), keys=keys.cpu().numpy().tobytes(), values=values.cpu().numpy().tobytes())


def check(seg_records, segs=None):
    """Plan and gather of the segments against the model of their concatenation; -> the model."""
    segs = segs or [Segment(r) for r in seg_records]
    want = WM.expected([r for recs in seg_records for r in recs])
    r = plan(segs)
    if want["result"][L.RIO_WAL_R_FIRST_BAD] != _NONE:
        assert r[L.RIO_WAL_R_FIRST_BAD:L.RIO_WAL_R_BAD_CLASS + 1] == want["result"][5:7]
        return want
    assert r == want["result"]
    n, kb, vb = r[L.RIO_WAL_R_N_OPS], r[L.RIO_WAL_R_KEY_BYTES], r[L.RIO_WAL_R_VALUE_BYTES]
    g = gather(n, kb, vb)
    for name in ("key_off", "val_off", "flags", "op_rec"):
        assert g[name] == want[name], name
    assert g["keys"] == want["keys"] + bytes([FILL]) * CANARY
    assert g["values"][:vb] == want["values"] and g["values"][vb:] == bytes([FILL]) * CANARY
    return want


# ---- record counts ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_record_counts(n):
    recs = WM.ordinary(random.Random(n), n)
    want = check([recs])
    assert want["result"][0] == n
    if n >= 255:
        assert 0 < want["result"][1] < n


def test_more_records_than_one_round_of_any_grid():
    """One record more than a full pass of the widest launch (the parse kernel's grid cap x 256 lanes; the copy
    kernels take 2 x 16 and 2 x 4 records per block and round), records of 2-6 bytes: every grid-stride loop goes
    round again."""
    n = max(GRID_CAP * 256, 2 * COPY_GRID_CAP * 256 // 16, 2 * COPY_GRID_CAP * 256 // 64) + 1
    pool = [b"\x0a\x00", b"\x12\x00", b"\x18\x01", b"\x1a\x01x", b"\x0a\x02\x0a\x00", b"\x0a\x04\x0a\x00\x12\x00"]
    for c in range(97, 123):
        k = bytes([c])
        pool += [P.marshal_upsert_str(k.decode(), ""), P.marshal_delete(k), P.marshal_delete(k + k), P.marshal_delete_str(k.decode())]
    assert all(2 <= len(r) <= 6 for r in pool)
    picks = np.random.default_rng(5).integers(0, len(pool), n).tolist()
    recs = [pool[i] for i in picks]
    want = check([recs])
    assert want["result"][0] == n and want["op_rec"][-1] >= GRID_CAP * 256 - 8


# ---- record kinds ----------------------------------------------------------------------------------------

def _kinds():
    ok = field(1, field(3, b"k") + field(4, b"v"))
    add, dele = field(1, field(3, b"ka") + field(4, b"va")), field(2, field(2, b"kd"))
    ten = lambda last: b"\x80" * 9 + bytes([last])  # noqa: E731
    return {
        "every kind": [P.marshal_upsert(b"kb", b"vb"), P.marshal_delete(b"kb"), P.marshal_upsert_str("ks", "vs"),
                       P.marshal_delete_str("ks"), None, b"", P.marshal_upsert(b"", b""), P.marshal_upsert_str("k", ""),
                       P.marshal_delete(b""), None, None, b""],
        "unknown fields": [field(3, b"u") + ok, field(1, field(9, b"u") + field(3, b"k") + field(4, b"v")) + field(2047, 5, 0),
                           field(77, b"only unknown")],
        "groups": [group(5, field(1, b"x") + group(6)) + ok, field(1, group(5, field(1, b"\xff")) + field(3, b"k") + field(4, b"v")),
                   nested_groups(16) + ok],
        "group depth 17": [ok, nested_groups(17) + ok],
        "unmatched group end": [ok, ok, P.put_varint(5 << 3 | 3) + P.put_varint(6 << 3 | 4)],
        "members with wire types 0, 1, 5": [field(1, 1, 0) + field(2, b"4444", 5) + field(1, b"88888888", 1) + ok,
                                            field(2, 9, 0), field(2, field(2, b"kd")) + field(1, 1, 0),
                                            field(1, field(3, 7, 0) + field(4, b"12345678", 1) + field(1, b"1234", 5))],
        "addition twice": [field(1, field(3, b"k1") + field(4, b"v1")) + field(1, field(4, b"v2") + field(1, b"s")),
                           field(1, field(1, b"s1")) + field(1, field(2, b"sv"))],
        "addition then delete": [add + dele, add + dele + field(1, field(4, b"only v"))],
        "delete then addition": [dele + add, field(2, field(1, b"a")) + field(2, field(2, b"b")) + field(2, b"")],
        "10-byte varint ending in 1": [b"\x08" + ten(1) + ok, field(1, b"\x28" + ten(1) + field(3, b"k") + field(4, b"v"))],
        "10-byte varint ending in 2": [ok, b"\x08" + ten(2) + ok],
        "10-byte varint ending in 2, inside": [field(1, b"\x28" + ten(2) + field(3, b"k") + field(4, b"v"))],
        "member leaves the record": [ok, ok, b"\x0a\x05\x1a\x01k"],
        "field leaves the member": [ok, b"\x0a\x03\x1a\x05k" + ok],
        "value nil": [ok, field(1, field(3, b"kb")), ok],
        "value nil, empty": [field(1, field(3, b"kb") + field(4, b"v") + field(4, b""))],
    }


@pytest.mark.parametrize("name", list(_kinds()))
def test_record_kinds(name):
    recs = _kinds()[name]
    want = check([recs])
    bad = {"group depth 17": (1, WM.PROTO), "unmatched group end": (2, WM.PROTO), "10-byte varint ending in 2": (1, WM.PROTO),
           "10-byte varint ending in 2, inside": (0, WM.PROTO), "member leaves the record": (2, WM.PROTO),
           "field leaves the member": (1, WM.PROTO), "value nil": (1, WM.VALUE_NIL), "value nil, empty": (0, WM.VALUE_NIL)}
    assert tuple(want["result"][5:7]) == bad.get(name, (_NONE, 0))


def test_seeded_corpus_families():
    c = WM.corpus(77, 400)
    check([c["ordinary"]])
    merged = WM.accepted(c["merges"])  # a merge can leave keyBytes without valueBytes: those go one at a time below
    assert 300 < len(merged) < 400
    check([merged])
    # refused records one at a time behind good ones, so each is the first refused record of its own plan
    good = c["ordinary"][:5]
    n_bad = 0
    for rec in [r for r in c["merges"] if r not in merged][:10] + c["malformed"][:60]:
        want = check([good + [rec] + good])
        n_bad += want["result"][5] != _NONE
    assert 15 < n_bad < 70


# ---- UTF-8 -----------------------------------------------------------------------------------------------

UTF8_BAD = [b"\xc0\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\x80", b"\xe2\x82"]


@pytest.mark.parametrize("s", UTF8_BAD, ids=lambda s: s.hex())
def test_invalid_utf8(s):
    ok = P.marshal_upsert_str("é€\U0001F600", "\ud7ff\ue000\uffff\U0010FFFF")  # the neighbours of what utf8.Valid refuses
    # the bad bytes end their record, so the 3-byte form cut short is cut at the record's end
    for rec in (field(1, field(1, s)), field(1, field(1, b"k") + field(2, s)), field(2, field(1, s)),
                field(1, field(1, s) + field(1, b"a later valid occurrence")) + field(1, field(2, s + b"!") + field(2, b"v" + s))):
        want = check([[ok, rec, ok]])
        assert want["result"][5:7] == [1, WM.UTF8]
    # the same bytes in keyBytes / valueBytes, and in a string field with another wire type, are not looked at
    recs = [ok, field(1, field(3, s) + field(4, s)), field(2, field(2, s)),
            field(1, field(1, b"\xff\xff\xff\xff", 5) + field(3, b"k") + field(4, b"v"))]
    want = check([recs])
    assert want["result"][5] == _NONE and (s, s) in want["ops"] and (s, None) in want["ops"]


# ---- lengths and alignments ------------------------------------------------------------------------------

def test_key_lengths():
    rng = random.Random(3)
    recs = []
    for n in (0, 1, 8, 9, 1024, 1025):
        k = rng.randbytes(n)
        recs += [P.marshal_upsert(k, b"v%d" % n) if n else P.marshal_upsert_str("", "v0"), P.marshal_delete(k),
                 P.marshal_upsert_str("s" * n, "x"), P.marshal_delete_str("t" * n)]
    want = check([recs])
    assert want["result"][L.RIO_WAL_R_MAX_KEY_LEN] == 1025 > L.RIO_FLUSH_MAX_KEY_LEN


def test_a_key_past_the_flush_limit_goes_through_the_plan_and_is_refused_by_recovery(tmp_path):
    wal_dir, table = _write_wal(tmp_path, [P.marshal_upsert(b"k", b"v"), P.marshal_upsert(b"K" * 1025, b"v")])
    before = sorted(os.listdir(wal_dir))
    n, wrote, err = DB.recover_wal(wal_dir, table)
    assert (n, wrote) == (2, False) and isinstance(err, S.UnsupportedError), err
    assert not os.path.exists(table) and sorted(os.listdir(wal_dir)) == before


def test_value_lengths():
    rng = random.Random(4)
    lens = [0, 1, 15, 16, 17, LONG_ITEM - 1, LONG_ITEM, LONG_ITEM + 1, 1 << 20]
    recs = [P.marshal_upsert(b"key %d" % n, rng.randbytes(n)) if n else P.marshal_upsert_str("key 0", "") for n in lens]
    recs += [P.marshal_upsert_str("str %d" % n, "s" * n) for n in lens[:-1]]
    want = check([recs])
    assert sorted({len(v) for _, v in want["ops"]}) == sorted(lens)


@pytest.mark.parametrize("long_items", [False, True])
def test_every_source_and_destination_alignment(long_items):
    """An op's key and value land at the sum of the lengths before them, and lie in the arena behind records of
    every length: with a first op of a = 0 .. 15 key and value bytes both addresses take every residue."""
    rng = random.Random(16)
    sizes = (LONG_ITEM, LONG_ITEM + 37, 3 * LONG_ITEM + 5) if long_items else (1, 15, 16, 17, 31, 33, 100)
    segs = []
    for a in range(16):
        recs = [P.marshal_upsert_str("k" * a, "v" * a)]
        for n in sizes:
            recs += [P.marshal_upsert(rng.randbytes(n), rng.randbytes(n + 1)), b"\x1a" + bytes([a % 3 + 1]) + b"xyz"[:a % 3 + 1]]
        segs.append(recs)
    for k in range(0, 16, 4):
        check(segs[k:k + 4])


# ---- segments --------------------------------------------------------------------------------------------

def _three(rng):
    return [WM.ordinary(rng, 300), WM.accepted(WM.merges(rng, 250))[:200], WM.ordinary(rng, 77)]


def test_one_and_three_segments():
    rng = random.Random(31)
    a, b, c = _three(rng)
    w1 = check([a + b + c])
    w3 = check([a, b, c])
    assert w1["op_rec"] == w3["op_rec"] and w3["result"][0] == 577


@pytest.mark.parametrize("where", ["first", "middle", "last", "all but one", "only empty"])
def test_empty_segments(where):
    a, b, c = _three(random.Random(32))
    shape = {"first": [[], [], a, b], "middle": [a, [], [], b, [], c], "last": [a, b, [], []],
             "all but one": [[], [], c, [], []], "only empty": [[], [], []]}[where]
    want = check(shape)
    assert want["result"][0] == sum(len(s) for s in shape)


def test_last_record_ends_exactly_at_the_arena_end():
    for last in (P.marshal_upsert(b"the last key", b"the last value" * 80), P.marshal_delete(b"the last key"),
                 field(1, field(3, b"k") + field(4, b"v")) + field(9, b"trailing unknown")):
        a = WM.ordinary(random.Random(33), 100)
        segs = [Segment(a), Segment(a[:50] + [last])]
        assert segs[1].c.out_bytes == sum(len(r or b"") for r in a[:50]) + len(last)
        check([a, a[:50] + [last]], segs)


# ---- bad records -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("first,second", [(WM.UTF8, WM.PROTO), (WM.PROTO, WM.UTF8), (WM.VALUE_NIL, WM.PROTO),
                                          (WM.PROTO, WM.VALUE_NIL)])
def test_two_bad_records_in_different_blocks(first, second):
    """Records 10 and 500 are handled by different workgroups (256 lanes each): the smaller index is reported,
    whichever class it has."""
    bad = {WM.PROTO: b"\x0a\x05\x1a\x01k", WM.UTF8: field(1, field(1, b"\xff")), WM.VALUE_NIL: field(1, field(3, b"k"))}
    recs = WM.ordinary(random.Random(41), 600)
    recs[10], recs[500] = bad[first], bad[second]
    assert plan([Segment(recs)])[5:7] == [10, first]
    assert check([recs])["result"][5:7] == [10, first]
    recs[10] = P.marshal_upsert(b"good", b"again")
    assert plan([Segment(recs)])[5:7] == [500, second]


def test_bad_record_in_a_later_segment_is_reported_by_its_global_index():
    a, b, c = _three(random.Random(42))
    c[40] = field(2, field(1, b"\xc0\x80"))
    want = check([a, [], b, c])
    assert want["result"][5:7] == [len(a) + len(b) + 40, WM.UTF8]


def test_inconsistent_offsets_give_bad_range():
    recs = WM.ordinary(random.Random(43), 300)
    good = np.cumsum([0] + [len(r or b"") for r in recs])
    total = int(good[-1])
    off = good.copy()
    assert off[149] > 0
    off[150] = off[149] - 1  # record 149 runs backwards
    r = plan([Segment(recs, off)])
    assert r[5:7] == [149, WM.RANGE]
    off = good.copy()
    off[300] = total + 1000  # the final offset is past the arena
    assert plan([Segment(recs, off)])[5:7] == [299, WM.RANGE]
    off = good.copy()
    off[200] = total + (1 << 40)  # far outside
    assert plan([Segment(recs, off)])[5:7] == [199, WM.RANGE]
    # an arena length shorter than the offsets: the first record that leaves it
    cut = int(good[120]) + 1
    first = next(i for i in range(300) if good[i + 1] > cut)
    assert plan([Segment(recs, good, out_bytes=cut)])[5:7] == [first, WM.RANGE]
    # in segment 2 of 3 the index is global, and the good log still plans as the model says
    assert plan([Segment(recs), Segment(recs, off), Segment(recs)])[5:7] == [300 + 199, WM.RANGE]
    check([recs])


# ---- caps ------------------------------------------------------------------------------------------------

def test_caps_one_byte_short():
    rng = random.Random(51)
    recs = WM.ordinary(rng, 200) + [P.marshal_upsert(b"a long last key " * 5, rng.randbytes(LONG_ITEM + 3))]
    want = check([recs])
    n, kb, vb = want["result"][1:4]
    lk, lv = len(want["ops"][-1][0]), len(want["ops"][-1][1])
    seg = Segment(recs)  # alive until the gathers have run
    for dk, dv in ((1, 0), (0, 1), (1, 1)):
        assert plan([seg]) == want["result"]
        g = gather(n, kb - dk, vb - dv)
        for name in ("key_off", "val_off", "flags", "op_rec"):
            assert g[name] == want[name], name
        # the last item would pass its cap: it is not copied, everything before it is; nothing past the cap is touched
        fill = bytes([FILL])
        keys = want["keys"][:kb - lk] + fill * (lk - 1) if dk else want["keys"]
        values = want["values"][:vb - lv] + fill * (lv - 1) if dv else want["values"]
        assert g["keys"] == keys + fill * CANARY
        assert g["values"] == values + fill * CANARY


def test_gather_without_op_rec_and_with_another_op_count():
    recs = WM.ordinary(random.Random(52), 300)
    want = check([recs])
    n, kb, vb = want["result"][1:4]
    seg = Segment(recs)  # alive until the gathers have run
    assert plan([seg]) == want["result"]
    g = gather(n, kb, vb, with_op_rec=False)
    assert g["key_off"] == want["key_off"] and g["keys"][:kb] == want["keys"] and g["op_rec"] == [-1] * n
    # fewer ops than the plan found: the first m, with their end offsets
    m = n - 7
    g = gather(m, kb, vb)
    assert g["key_off"] == want["key_off"][:m + 1] and g["val_off"] == want["val_off"][:m + 1]
    assert g["flags"] == want["flags"][:m] and g["op_rec"] == want["op_rec"][:m]
    assert g["keys"][:want["key_off"][m]] == want["keys"][:want["key_off"][m]]
    assert g["keys"][want["key_off"][m]:] == bytes([FILL]) * (kb - want["key_off"][m] + CANARY)
    # more (up to the record count): empty tombstones behind the plan's ops
    g = gather(n + 3, kb, vb)
    assert g["key_off"] == want["key_off"] + [kb] * 3 and g["val_off"] == want["val_off"] + [vb] * 3
    assert g["flags"] == want["flags"] + [L.RIO_FLAG_NIL] * 3 and g["op_rec"][n:] == [-1] * 3
    p = torch.zeros(8, dtype=torch.int64, device="cuda").data_ptr()  # refused on the count, before any use
    assert L.lib().rio_wal_ops_gather(L.default_ctx(0), len(recs) + 1, p, 0, p, p, 0, p, p, None, None) == L.RIO_ERR_ARG


# ---- end to end ------------------------------------------------------------------------------------------

def _write_wal(tmp_path, records, max_size=64 << 10):
    wal_dir, table = str(tmp_path / "wal"), str(tmp_path / "table")
    os.makedirs(wal_dir)
    opts, err = W.NewWriteAheadLogOptions(W.BasePath(wal_dir), W.MaximumWalFileSizeBytes(max_size),
                                          W.WriterFactory(lambda p: __import__("recordio").NewFileWriter(p, L.COMP_SNAPPY)))
    assert err is None, err
    a, err = W.NewAppender(opts)
    assert err is None, err
    for rec in records:
        assert a.Append(rec) is None
    assert a.Close() is None
    return wal_dir, table


def _workload(seed, n_ops=5000):
    """About n_ops ops on 700 keys (so keys repeat), tombstones and re-inserts, empty records in between."""
    rng = random.Random(seed)
    recs = []
    for i in range(n_ops):
        key = b"user/%05d" % rng.randrange(700)
        r = rng.random()
        if r < 0.70:
            recs.append(P.marshal_upsert(key, rng.randbytes(rng.randint(1, 120)) + b"#%d" % i))
        elif r < 0.85:
            recs.append(P.marshal_delete(key))
        elif r < 0.93:
            recs.append(P.marshal_upsert_str(key.decode(), "text value %d" % i))
        else:
            recs.append(P.marshal_delete_str(key.decode()))
        if i % 9 == 0:
            recs.append(b"")
    return recs


@pytest.fixture(scope="module")
def workload():
    recs = _workload(61)
    ops, _, first_bad, _ = WM.replay(recs)
    assert first_bad == _NONE and len(ops) == 5000
    return recs, ops


def _snapshot(d):
    return {name: open(os.path.join(d, name), "rb").read() for name in sorted(os.listdir(d))}


def test_recover_wal_writes_the_models_table(tmp_path, workload):
    recs, ops = workload
    wal_dir, table = _write_wal(tmp_path, recs)
    assert len(os.listdir(wal_dir)) >= 3
    n, wrote, err = DB.recover_wal(wal_dir, table)
    assert err is None, err
    assert (n, wrote) == (len(recs), True)
    want = str(tmp_path / "want")
    pairs, meta = FM.write_expected(want, ops, FM.WITH_TOMBSTONES)
    for name in FM.FILES:
        assert open(os.path.join(table, name), "rb").read() == open(os.path.join(want, name), "rb").read(), name
    r, err = S.NewSSTableReader(S.ReadBasePath(table))
    assert err is None, err
    assert scan_all(r) == pairs and r.MetaData().numRecords == len(pairs) == meta.numRecords
    assert any(v is None for _, v in pairs) and r.MetaData().nullValues == sum(v is None for _, v in pairs)
    assert os.path.isdir(wal_dir) and os.listdir(wal_dir) == []


@pytest.mark.parametrize("cls", [WM.PROTO, WM.UTF8, WM.VALUE_NIL])
def test_recover_wal_stops_at_a_bad_record(tmp_path, workload, cls):
    recs = list(workload[0])
    bad = {WM.PROTO: (b"\x0a\x05\x1a\x01k", "proto: cannot parse invalid wire-format data"),
           WM.UTF8: (field(1, field(1, b"k") + field(2, b"\xed\xa0\x80")),
                     "proto: field proto.UpsertMutation.value contains invalid UTF-8"),
           WM.VALUE_NIL: (field(1, field(3, b"k")), "value was nil")}[cls]
    at = 3333
    recs[at] = bad[0]
    wal_dir, table = _write_wal(tmp_path, recs)
    files = sorted(os.listdir(wal_dir))
    before = _snapshot(wal_dir)
    # the file that holds record `at`, by the files' record counts
    seen, path = 0, None
    for name in files:
        k = gpu_util.gpu_decode_arrays(before[name])["n_records"]
        if seen <= at < seen + k:
            path = os.path.join(wal_dir, name)
        seen += k
    assert seen == len(recs) and path not in (None, os.path.join(wal_dir, files[0]))
    n, wrote, err = DB.recover_wal(wal_dir, table)
    assert wrote is False and err is not None
    assert str(err) == f"error while processing WAL record under '{path}': {bad[1]}"
    if cls == WM.VALUE_NIL:
        assert err.wrapped is MS.ValueNil and n == at + 1
    else:
        assert n == at
    assert not os.path.exists(table) and _snapshot(wal_dir) == before


def test_recover_wal_of_no_ops_writes_no_table(tmp_path):
    recs = [b"", field(9, b"unknown"), b"", field(1, 1, 0)] * 25
    wal_dir, table = _write_wal(tmp_path, recs, 256)
    assert len(os.listdir(wal_dir)) >= 3
    assert DB.recover_wal(wal_dir, table) == (100, False, None)
    assert not os.path.exists(table) and os.listdir(wal_dir) == []
    assert DB.recover_wal(wal_dir, table) == (0, False, None)  # the fresh directory


def test_a_bad_record_comes_before_a_later_files_read_error(tmp_path, workload):
    recs = list(workload[0][:2000])
    recs[100] = b"\x0f"
    wal_dir, table = _write_wal(tmp_path, recs, 16 << 10)
    files = sorted(os.listdir(wal_dir))
    assert len(files) >= 3
    first, last = os.path.join(wal_dir, files[0]), os.path.join(wal_dir, files[-1])
    img = bytearray(open(last, "rb").read())
    img[8] ^= 0xFF  # the last file's first record header loses its magic number
    open(last, "wb").write(bytes(img))
    before = _snapshot(wal_dir)
    n, wrote, err = DB.recover_wal(wal_dir, table)
    assert (n, wrote) == (100, False)
    assert str(err) == f"error while processing WAL record under '{first}': proto: cannot parse invalid wire-format data"
    # without the bad record the read error is what recovery returns
    recs[100] = b""
    wal2 = tmp_path / "second"
    wal2.mkdir()
    wal_dir2, table2 = _write_wal(wal2, recs, 16 << 10)
    last2 = os.path.join(wal_dir2, sorted(os.listdir(wal_dir2))[-1])
    img = bytearray(open(last2, "rb").read())
    img[8] ^= 0xFF
    open(last2, "wb").write(bytes(img))
    n, wrote, err = DB.recover_wal(wal_dir2, table2)
    assert wrote is False and str(err).startswith(f"error while reading WAL records under '{last2}': ")
    assert not os.path.exists(table) and not os.path.exists(table2) and _snapshot(wal_dir) == before
