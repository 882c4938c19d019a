"""SuperSSTableReader on the device (GPU): rio_sst_stack_* and rio_sst_keys_gather (csrc/rio_stack.hip) and the
mirror (sstables/super_reader.py). Every result is compared with the stack model (tests/super_model.py) and with
SuperSSTableReader.Get / Contains, which are the reference's loops over the readers' single-key calls."""
import ctypes
import os
import shutil
import struct

import numpy as np
import pytest
import torch

import sstables as S
import super_model as sm
from conftest import GOLDEN
from recordio import _lib as L
from sstables import bloom
from sstables.writer import write_sstable

pytestmark = pytest.mark.gpu

_NONE = 0xFFFFFFFFFFFFFFFF
BITS = L.RIO_MERGE_ENTRY_BITS
K_LONG = 1024  # kLongItem (rio_seg_copy.h): values and keys from this length on are copied by a whole wave
P8 = b"prefix_8"


def be(i):
    return struct.pack(">I", i)


def val(n, seed):
    return bytes((seed * 31 + 7 * j) & 0xFF for j in range(n))


def open_stack(tmp_path, tables, blooms=(), opts=(), name="t", **kw):
    """One table per dict (oldest first), written by the host writer; tables in `blooms` get a filter."""
    readers = []
    for i, t in enumerate(tables):
        base = str(tmp_path / f"{name}{i}")
        wopts = (S.EnableBloomFilter(), S.BloomExpectedNumberOfElements(max(len(t), 1))) if i in blooms else ()
        write_sstable(base, sorted(t.items()), writer_options=wopts)
        r, err = S.NewSSTableReader(S.ReadBasePath(base), *opts)
        assert err is None, err
        readers.append(r)
    return S.NewSuperSSTableReader(readers, **kw)


def same(batch, loop):
    assert len(batch) == len(loop)
    for i, ((bv, berr), (lv, lerr)) in enumerate(zip(batch, loop)):
        assert bv == lv and type(bv) is type(lv), i
        assert (berr is None) == (lerr is None) and str(berr) == str(lerr), i
        assert (berr is S.NotFound) == (lerr is S.NotFound), i


def check(sr, model, queries, filters_hold_their_keys=True):
    """GetBatch / ContainsBatch == the loops of Get / Contains == the model; the source words name the newest table."""
    gets = [sr.Get(q) for q in queries]
    same(sr.GetBatch(queries), gets)
    same(sr.ContainsBatch(queries), [sr.Contains(q) for q in queries])
    for q, (v, err) in zip(queries, gets):
        want = model.get(q)
        assert (v, err) == ((None, S.NotFound) if want is sm.NOT_FOUND else (want, None)), q
    if filters_hold_their_keys:
        assert [f for f, _ in sr.ContainsBatch(queries)] == [model.contains(q) for q in queries]
    src, status, val_off, values = on_device(sr, queries)
    for q, w, s in zip(queries, src, status):
        where = model.source(q)
        assert w == (_NONE if where is None else (where[0] << BITS) | where[1]), q
        want = model.get(q)
        assert s == (L.RIO_GET_NOT_FOUND if want is sm.NOT_FOUND else L.RIO_GET_NIL if want is None else L.RIO_GET_VALUE)
    want_vals = [v for v in (model.get(q) for q in queries) if v is not sm.NOT_FOUND and v is not None]
    assert values == b"".join(want_vals) and val_off[-1] == len(values)
    return gets


def arena(queries):
    raw = b"".join(queries)
    d_keys = torch.from_numpy(np.frombuffer(raw or b"\0", dtype=np.uint8).copy()).cuda()
    d_off = torch.from_numpy(np.cumsum([0] + [len(q) for q in queries]).astype(np.int64)).cuda()
    return d_keys, d_off, len(raw)


def on_device(sr, queries):
    d_keys, d_off, nbytes = arena(queries)
    src, status, val_off, values = sr.GetBatchOnDevice(d_keys, d_off, len(queries))
    torch.cuda.synchronize()
    return ([x & _NONE for x in src.cpu().tolist()], status.cpu().tolist(), val_off.cpu().tolist(),
            bytes(values.cpu().numpy()))


# ---- stack shapes, key places and key forms ------------------------------------------------------------------------

FORMS = [b"", b"a", b"a\0", b"a\0\0", b"ab", b"ab\0\0\0\0\0\0", b"ab\0\0\0\0\0\0\0", P8, P8 + b"\0", P8 + b"x", P8 + b"y",
         P8 + b"xx", b"prefix_", b"\xff\xff"]


def forms_tables():
    """Five tables, oldest first: a table of key forms, an EMPTY table in the middle, a single-entry table, ..."""
    return [
        {k: b"old:" + k for k in FORMS} | {be(7): b"only-oldest", be(8): b"two-oldest-0", be(9): b"every-0"},
        {be(8): b"two-oldest-1", be(9): b"every-1", P8 + b"y": b"", b"a\0": None},
        {},
        {be(9): b"every-3"},
        {be(9): b"every-4", P8 + b"x": b"newest", b"ab\0\0\0\0\0\0": b"padded-twin"},
    ]


@pytest.mark.parametrize("blooms", [(), (0, 1, 2, 3, 4), (1, 4)], ids=["plain", "filters", "mixed"])
def test_key_places_and_forms(tmp_path, blooms):
    tables = forms_tables()
    sr = open_stack(tmp_path, tables, blooms)
    model = sm.Stack(tables)
    queries = FORMS + [be(7), be(8), be(9), be(6), be(10), b"\0", b"\xff\xff\xff", b"absent", P8 + b"z", P8[:7] + b"9",
                       b"a\0\0\0", b"ab\0", be(9), be(9)]
    gets = check(sr, model, queries)
    assert gets[queries.index(b"a\0")] == (None, None)        # nil in the newer table: no fall-through to "old:a\0"
    assert gets[queries.index(P8 + b"y")] == (b"", None)      # empty, not nil
    assert gets[queries.index(be(9))] == (b"every-4", None) and gets[queries.index(be(7))] == (b"only-oldest", None)
    assert gets[queries.index(be(8))] == (b"two-oldest-1", None)
    assert sr.Contains(b"a\0") == (True, None)
    assert sr.Close() is None


@pytest.mark.parametrize("T", [1, 2, L.RIO_MERGE_MAX_TABLES])
def test_stack_heights(tmp_path, T):
    """Tables of 0 to 3 entries. The tallest stack opens 16 tables and stands each at 16 positions: the views are
    copied per position, and the source word must name the highest position that holds the key."""
    distinct = [{be(10 * (i % 5) + j): b"t%d-%d" % (i, j) for j in range(i % 4)} for i in range(min(T, 16))]
    base = open_stack(tmp_path, distinct)
    readers = [base.readers[p % len(distinct)] for p in range(T)]
    tables = [distinct[p % len(distinct)] for p in range(T)]
    sr = S.NewSuperSSTableReader(readers)
    queries = [be(i) for i in range(0, 50)] + [b""]
    check(sr, sm.Stack(tables), queries)
    sr._free_stack()


# ---- values --------------------------------------------------------------------------------------------------------

LENGTHS = (0, 1, 15, 16, 17, 31, 33, K_LONG - 1, K_LONG, K_LONG + 1, 4097)


def test_value_lengths_at_every_destination_residue(tmp_path):
    """Every length starts at every destination residue mod 16: each is followed by a pad value whose length
    brings the next start one byte further. The same keys recur in the batch."""
    newest = {b"v%04d" % n: val(n, n) for n in LENGTHS}
    pads = {b"pad%02d" % n: val(n, 100 + n) for n in range(1, 17)}
    older = {b"v%04d" % n: b"stale" for n in LENGTHS} | pads
    sr = open_stack(tmp_path, [older, newest])
    model = sm.Stack([older, newest])
    queries, starts, off = [], {n: set() for n in LENGTHS}, 0
    for n in LENGTHS:
        for _ in range(16):
            pad = (1 - n) % 16 or 16
            queries += [b"v%04d" % n, b"pad%02d" % pad]
            starts[n].add(off % 16)
            off += n + pad
    assert all(len(s) == 16 for s in starts.values())
    check(sr, model, queries)
    # the value arena is 256-byte aligned (a fresh tensor), so the offsets are the addresses' residues
    src, status, val_off, values = sr.GetBatchOnDevice(*arena(queries)[:2], len(queries))
    assert values.data_ptr() % 256 == 0 and {int(x) % 16 for x in val_off[:-1:2].cpu().tolist()} == set(range(16))
    sr._free_stack()


def test_values_cap_one_byte_short_and_hostile_source_words(tmp_path):
    tables = [{be(1): b"one", be(2): b"twotwo"}, {be(3): val(40, 3), be(4): None}]
    sr = open_stack(tmp_path, tables)
    queries = [be(1), be(3), be(2)]
    src, status, val_off, values = sr.GetBatchOnDevice(*arena(queries)[:2], 3)
    lib, n = L.lib(), 3
    total = int(val_off[n].item())
    assert total == 3 + 40 + 6
    out = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    rc = lib.rio_sst_stack_value_copy(sr._stack, src.data_ptr(), n, val_off.data_ptr(), out.data_ptr(), total - 1, None)
    assert rc == L.RIO_OK
    torch.cuda.synchronize()
    got = bytes(out.cpu().numpy())
    assert got[:43] == b"one" + val(40, 3) and got[43:] == b"\xEE" * (6 + 64)  # the last value is not copied
    # source words that name no entry: a table >= T, an entry >= n, ~0, all bits but the top; then two good ones
    words = [(2 << BITS) | 0, (1 << BITS) | 2, _NONE, _NONE >> 1, (0 << BITS) | 5, (1 << BITS) | 0, (1 << BITS) | 1]
    d_src = torch.from_numpy(np.array(words, dtype=np.uint64).view(np.int64)).cuda()
    st = torch.full((len(words),), 0xEE, dtype=torch.uint8, device="cuda")
    vo = torch.full((len(words) + 1,), -1, dtype=torch.int64, device="cuda")
    assert lib.rio_sst_stack_value_plan(sr._stack, d_src.data_ptr(), len(words), 1, st.data_ptr(), vo.data_ptr(), None) == 0
    out.fill_(0xEE)
    assert lib.rio_sst_stack_value_copy(sr._stack, d_src.data_ptr(), len(words), vo.data_ptr(), out.data_ptr(), 64, None) == 0
    torch.cuda.synchronize()
    NF = L.RIO_GET_NOT_FOUND
    assert st.cpu().tolist() == [NF, NF, NF, NF, NF, L.RIO_GET_VALUE, L.RIO_GET_NIL]
    assert vo.cpu().tolist() == [0, 0, 0, 0, 0, 0, 40, 40]
    assert bytes(out.cpu().numpy())[:41] == val(40, 3) + b"\xEE"
    sr._free_stack()


# ---- batch sizes ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_batch_sizes(tmp_path, n):
    tables = [{be(i): b"o%d" % i for i in range(0, 300, 2)}, {be(i): b"n%d" % i for i in range(0, 300, 3)}]
    sr = open_stack(tmp_path, tables, blooms=(0,))
    check(sr, sm.Stack(tables), [be(i) for i in range(n)])
    assert sr.GetBatch([]) == [] and sr.ContainsBatch([]) == []
    sr._free_stack()


def test_one_query_past_a_full_round_of_the_grid(tmp_path):
    n = 2048 * 256 + 1  # kStackGridCap blocks of 256 lanes, and one more query
    tables = [{be(5): b"five", be(n - 1): b"old-last"}, {be(n - 1): b"last", be(70000): b""}]
    sr = open_stack(tmp_path, tables)
    rows = np.arange(n, dtype=">u4").view(np.uint8).reshape(-1)
    d_keys = torch.from_numpy(rows.copy()).cuda()
    d_off = torch.from_numpy(4 * np.arange(n + 1, dtype=np.int64)).cuda()
    src, status, val_off, values = sr.GetBatchOnDevice(d_keys, d_off, n)
    torch.cuda.synchronize()
    want = np.full(n, -1, dtype=np.int64)
    want[5], want[70000], want[n - 1] = (0 << BITS) | 0, (1 << BITS) | 0, (1 << BITS) | 1  # be(70000) sorts first
    np.testing.assert_array_equal(src.cpu().numpy(), want)
    st = np.full(n, L.RIO_GET_NOT_FOUND, dtype=np.uint8)
    st[5] = st[70000] = st[n - 1] = L.RIO_GET_VALUE
    np.testing.assert_array_equal(status.cpu().numpy(), st)
    assert bytes(values.cpu().numpy()) == b"fivelast" and int(val_off[n].item()) == 8 and int(val_off[n - 1].item()) == 4
    sr._free_stack()


def test_a_batch_larger_than_max_batch_is_split_by_the_mirror(tmp_path):
    tables = [{be(i): b"o%d" % i for i in range(0, 40, 2)}, {be(i): None if i % 9 == 0 else b"n%d" % i for i in range(0, 40, 3)}]
    sr = open_stack(tmp_path, tables, max_batch=7)
    queries = [be(i) for i in range(45)]
    same(sr.GetBatch(queries), [sr.Get(q) for q in queries])
    same(sr.ContainsBatch(queries), [sr.Contains(q) for q in queries])
    d_keys, d_off, nbytes = arena(queries[:8])
    out = torch.zeros(8, dtype=torch.int64, device="cuda")
    lib = L.lib()
    assert lib.rio_sst_stack_lookup(sr._stack, 0, d_keys.data_ptr(), d_off.data_ptr(), 8, nbytes, out.data_ptr(), None) == L.RIO_ERR_ARG
    assert lib.rio_sst_stack_lookup(sr._stack, 0, d_keys.data_ptr(), d_off.data_ptr(), 7, nbytes, out.data_ptr(), None) == L.RIO_OK
    assert lib.rio_sst_stack_value_plan(sr._stack, out.data_ptr(), 8, 0, d_keys.data_ptr(), out.data_ptr(), None) == L.RIO_ERR_ARG
    torch.cuda.synchronize()
    sr._free_stack()


# ---- the gate ------------------------------------------------------------------------------------------------------

def test_a_filter_built_for_other_keys(tmp_path):
    """Contains follows the table's filter, as the reference does (sstable_reader.go:49-65); Get asks none."""
    old = {be(i): b"old%d" % i for i in range(0, 60)}
    new = {be(i): b"new%d" % i for i in range(0, 60, 2)}
    other = {be(1000 + i): b"x" for i in range(30)}
    write_sstable(str(tmp_path / "other"), sorted(other.items()),
                  writer_options=(S.EnableBloomFilter(), S.BloomExpectedNumberOfElements(30)))
    write_sstable(str(tmp_path / "n0"), sorted(old.items()))
    write_sstable(str(tmp_path / "n1"), sorted(new.items()))
    shutil.copy(str(tmp_path / "other" / "bloom.bf.gz"), str(tmp_path / "n1" / "bloom.bf.gz"))
    readers = [S.NewSSTableReader(S.ReadBasePath(str(tmp_path / d)))[0] for d in ("n0", "n1")]
    assert readers[0].bloomFilter is None and readers[1].bloomFilter is not None
    sr = S.NewSuperSSTableReader(readers)
    queries = [be(i) for i in range(0, 70)] + [be(1000 + i) for i in range(5)]
    same(sr.GetBatch(queries), [sr.Get(q) for q in queries])
    same(sr.ContainsBatch(queries), [sr.Contains(q) for q in queries])
    assert sr.GetBatch([be(2)]) == [(b"new2", None)]
    # the newer table's filter rejects (nearly) all of its own keys: gated, such a key is found in the older table
    d_keys, d_off, nbytes = arena(queries)
    gated = torch.zeros(len(queries), dtype=torch.int64, device="cuda")
    assert L.lib().rio_sst_stack_lookup(sr._stack, 1, d_keys.data_ptr(), d_off.data_ptr(), len(queries), nbytes,
                                        gated.data_ptr(), None) == L.RIO_OK
    torch.cuda.synchronize()
    f = readers[1].bloomFilter
    want = [(1 << BITS) | (i // 2) if i < 60 and i % 2 == 0 and f.Contains(be(i)) else (i if i < 60 else _NONE)
            for i in list(range(70)) + [1000 + i for i in range(5)]]
    assert [x & _NONE for x in gated.cpu().tolist()] == want
    assert sum(w >> BITS == 0 for w in want[:60:2]) > 20
    sr._free_stack()


def test_a_filter_with_65_probes(tmp_path):
    tables = [{be(i): b"v%d" % i for i in range(10)}, {be(i): b"w%d" % i for i in range(5, 15)}]
    for i, t in enumerate(tables):
        write_sstable(str(tmp_path / f"t{i}"), sorted(t.items()))
    f, err = bloom.New(4096, 65)
    assert err is None
    for k in tables[1]:
        f.Add(k)
    assert f.WriteFile(str(tmp_path / "t1" / "bloom.bf.gz")) is None
    readers = [S.NewSSTableReader(S.ReadBasePath(str(tmp_path / f"t{i}")))[0] for i in range(2)]
    assert readers[1].bloomFilter.k == 65
    sr = S.NewSuperSSTableReader(readers)
    queries = [be(i) for i in range(20)]
    got = sr.ContainsBatch(queries)
    assert all(found is False and isinstance(e, S.UnsupportedError) and "65 probes" in str(e) for found, e in got)
    same(got[:1], readers[1].ContainsBatch(queries[:1]))  # the single table's refusal
    same(sr.GetBatch(queries), [sr.Get(q) for q in queries])
    assert [sr.Contains(q) for q in queries] == [(i < 15, None) for i in range(20)]
    sr._free_stack()


# ---- errors --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("check_reads", [False, True])
def test_a_value_that_fails_its_checksum(tmp_path, check_reads):
    """The reference's CRCHashesMismatch table (its fourth value has a flipped byte) as the newest of two."""
    older = {be(i): b"good%d" % i for i in range(0, 10)}
    write_sstable(str(tmp_path / "older"), sorted(older.items()))
    ropts = (S.EnableHashCheckOnReads(),) if check_reads else ()
    r0, err = S.NewSSTableReader(S.ReadBasePath(str(tmp_path / "older")), *ropts)
    assert err is None, err
    r1, err = S.NewSSTableReader(S.ReadBasePath(os.path.join(GOLDEN, "sstables", "SimpleWriteHappyPathSSTableWithCRCHashesMismatch")),
                                 S.SkipHashCheckOnLoad(), *ropts)
    assert err is None, err
    sr = S.NewSuperSSTableReader([r0, r1])
    queries = [be(i) for i in range(0, 12)]
    gets = [sr.Get(q) for q in queries]
    same(sr.GetBatch(queries), gets)
    if check_reads:  # the newer table's error is returned although the older table holds a good value
        assert gets[4][0] is None and "Checksum mismatch: expected 688fffff90000000, got 738fffff90000000" in str(gets[4][1])
        it, err = sr.Scan()
        assert it is None and isinstance(err, S.UnsupportedError) and "fails its checksum" in str(err)
    else:
        assert gets[4] == (be(0x15), None)
        it, err = sr.Scan()
        assert err is None and drain(it)[4] == (be(4), be(0x15))
    assert [e for _, e in gets[:4] + gets[5:10]] == [None] * 9 and gets[0] == (b"good0", None) and gets[1] == (be(2), None)
    src, status, _, _ = on_device(sr, queries)
    assert status[4] == (L.RIO_GET_HOST if check_reads else L.RIO_GET_VALUE) and src[4] == (1 << BITS) | 3
    sr._free_stack()


def test_a_record_that_does_not_decompress(tmp_path):
    older = {b"k%d" % i: b"fine" for i in range(5)}
    newer = {b"k%d" % i: b"x" * 100 for i in range(5)}
    write_sstable(str(tmp_path / "t0"), sorted(older.items()))
    write_sstable(str(tmp_path / "t1"), sorted(newer.items()))
    p = str(tmp_path / "t1" / "data.rio")
    img = bytearray(open(p, "rb").read())
    img[-3:] = b"\xff\xff\xff"  # the last record's last Snappy element becomes a copy that needs five bytes
    open(p, "wb").write(img)
    readers = [S.NewSSTableReader(S.ReadBasePath(str(tmp_path / f"t{i}")), S.SkipHashCheckOnLoad())[0] for i in range(2)]
    assert readers[1] is not None and readers[1].t.value_bad == 4
    sr = S.NewSuperSSTableReader(readers)
    queries = [b"k%d" % i for i in range(6)]
    gets = [sr.Get(q) for q in queries]
    same(sr.GetBatch(queries), gets)
    assert gets[4][0] is None and "failed decompressing record at offset" in str(gets[4][1])
    assert gets[3] == (b"x" * 100, None) and gets[5] == (None, S.NotFound)
    assert on_device(sr, queries)[1] == [L.RIO_GET_VALUE] * 4 + [L.RIO_GET_HOST, L.RIO_GET_NOT_FOUND]
    it, err = sr.ScanRange(b"k0", b"k1")
    assert it is None and isinstance(err, S.UnsupportedError) and "cannot be read" in str(err)
    sr._free_stack()


def test_v0_tables_answer_by_the_host_loop():
    base = os.path.join(GOLDEN, "sstables_v0_compat", "SimpleWriteHappyPathSSTableWithMetaData")
    r0, err = S.NewSSTableReader(S.ReadBasePath(base))
    assert err is None and r0.t.v0
    r1, err = S.NewSSTableReader(S.ReadBasePath(os.path.join(GOLDEN, "sstables", "SimpleWriteHappyPathSSTableWithCRCHashes")))
    assert err is None
    sr = S.NewSuperSSTableReader([r0, r1])
    queries = [be(i) for i in range(0, 9)]
    same(sr.GetBatch(queries), [sr.Get(q) for q in queries])
    same(sr.ContainsBatch(queries), [sr.Contains(q) for q in queries])
    it, err = sr.Scan()
    assert it is None and isinstance(err, S.UnsupportedError) and "v0 tables" in str(err)
    # v0 values are DataEntry ranges inside the records: the device value path refuses the stack, it does not
    # hand out the records' wire bytes
    with pytest.raises(S.UnsupportedError, match="v0 table"):
        sr.GetBatchOnDevice(*arena(queries)[:2], len(queries))
    sr._free_stack()


# ---- scans ---------------------------------------------------------------------------------------------------------

def drain(it):
    out = []
    while True:
        k, v, err = it.Next()
        if err is S.Done:
            assert it.Next()[2] is S.Done
            return out
        assert err is None, err
        out.append((k, v))


def device_items(scan):
    keys, key_off, values, val_off, flags, n = scan
    torch.cuda.synchronize()
    hk, hv = bytes(keys.cpu().numpy()), bytes(values.cpu().numpy())
    ko, vo = key_off.cpu().tolist(), val_off.cpu().tolist()
    assert len(ko) == n + 1 and len(vo) == n + 1 and not flags.cpu().numpy().any()
    return [(hk[ko[j]:ko[j + 1]], hv[vo[j]:vo[j + 1]]) for j in range(n)]


def scan_tables():
    run = {P8 + bytes([c]): b"run%d" % c for c in range(0x61, 0x69)}  # equal 8-byte prefixes
    return [
        {be(i): b"a%d" % i for i in range(0, 40, 2)} | run | {b"": b"empty-key", b"k" * 1500: b"long-key"},
        {},
        {be(i): None if i % 4 == 0 else b"" if i % 4 == 1 else val(i * 37 % 1300, i) for i in range(0, 40, 3)},
        {be(50): b"only"},
        {P8 + b"c": None, P8 + b"e": b"newest-e", be(39): b"thirty-nine"},
    ]


def test_scans_equal_the_model(tmp_path):
    tables = scan_tables()
    sr = open_stack(tmp_path, tables, blooms=(0,))
    model = sm.Stack(tables)
    every = model.scan()
    assert (be(0), b"a0") not in every and (be(9), b"") in every and (P8 + b"c") not in dict(every)  # nil drops, empty stays
    it, err = sr.Scan()
    assert err is None and drain(it) == every
    scan, err = sr.ScanOnDevice()
    assert err is None and device_items(scan) == every
    last = every[-1][0]
    for key in (be(10), be(11), b"", b"\0", last, last + b"\0", b"\xff" * 3, P8 + b"c", P8 + b"cc", P8):
        it, err = sr.ScanStartingAt(key)
        assert err is None and drain(it) == model.scan(key), key
        scan, err = sr.ScanStartingAtOnDevice(key)
        assert err is None and device_items(scan) == model.scan(key), key
    it, _ = sr.ScanStartingAt(last + b"\0")
    assert it.Next() == (None, None, S.Done)  # above the last key: the first Next is Done
    ranges = [(be(10), be(10)), (be(11), be(11)), (be(3), be(3)), (be(50), be(50)), (be(41), be(49)), (be(60), be(70)),
              (P8 + b"b", P8 + b"f"), (P8 + b"bb", P8 + b"e"), (P8, P8 + b"\xff"), (b"", b""), (b"", b"\xff" * 4),
              (be(0), be(39)), (b"k" * 1499, b"k" * 1501)]
    for lo, hi in ranges:
        it, err = sr.ScanRange(lo, hi)
        assert err is None and drain(it) == model.scan(lo, hi), (lo, hi)
        scan, err = sr.ScanRangeOnDevice(lo, hi)
        assert err is None and device_items(scan) == model.scan(lo, hi), (lo, hi)
    assert model.scan(be(41), be(49)) == [] and model.scan(be(50), be(50)) == [(be(50), b"only")]
    # lo > hi: the first reader's error
    it, err = sr.ScanRange(be(5), be(4))
    _, want = sr.readers[0].ScanRange(be(5), be(4))
    assert it is None and str(err) == str(want) and "keyHigher is lower than keyLower" in str(err)
    # each table's iterator alone agrees with the cut the stack made for it
    for t, r in enumerate(sr.readers):
        one = S.NewSuperSSTableReader([r])
        it, err = one.ScanRange(be(3), P8 + b"d")
        assert err is None and drain(it) == sm.Stack([tables[t]]).scan(be(3), P8 + b"d")
        one._free_stack()
    sr._free_stack()


def test_scanned_keys_at_the_copy_class_boundary(tmp_path):
    """k_keys_copy's two instantiations meet at K_LONG, and a key ends its 16-byte words at 15, 16 and 17 bytes."""
    lens = (15, 16, 17, K_LONG - 1, K_LONG, K_LONG + 1)
    tables = [{bytes([0x41 + j]) * n: b"old%d" % n for j, n in enumerate(lens)} | {b"B" * K_LONG: None},
              {bytes([0x61 + j]) * n: val(n % 40, n) for j, n in enumerate(lens)} | {b"B" * 16: b"newer"}]
    sr = open_stack(tmp_path, tables)
    model = sm.Stack(tables)
    every = model.scan()
    assert sorted(len(k) for k, _ in every) == sorted(lens + lens) and (b"B" * 16, b"newer") in every  # the nil key drops
    scan, err = sr.ScanOnDevice()
    assert err is None and device_items(scan) == every
    for lo, hi in ((b"C" * (K_LONG - 1), b"b" * 16), (b"E" * K_LONG, b"E" * K_LONG), (b"a", b"f" * (K_LONG + 1))):
        scan, err = sr.ScanRangeOnDevice(lo, hi)
        assert err is None and device_items(scan) == model.scan(lo, hi) and model.scan(lo, hi), (lo, hi)
    sr._free_stack()


def test_below_every_first_key(tmp_path):
    """No table stores the empty key: queries and scan starts below the first key of every table."""
    tables = [{be(5): b"five", be(9): b"nine-old"}, {}, {be(7): None, be(9): b"nine"}, {be(6): b"six"}]
    sr = open_stack(tmp_path, tables, blooms=(0,))
    model = sm.Stack(tables)
    check(sr, model, [b"", b"\0", b"\0\0\0", be(4), be(4) + b"\xff", be(5), be(6)])
    every = [(be(5), b"five"), (be(6), b"six"), (be(9), b"nine")]
    assert model.scan() == every
    for key in (b"", b"\0", b"\0\0\0", be(4), be(4) + b"\xff"):
        it, err = sr.ScanStartingAt(key)
        assert err is None and drain(it) == every, key
        scan, err = sr.ScanStartingAtOnDevice(key)
        assert err is None and device_items(scan) == every, key
        it, err = sr.ScanRange(key, be(6))
        assert err is None and drain(it) == every[:2], key
    it, err = sr.ScanRange(b"", be(4))  # a range wholly below the first key
    assert err is None and it.Next() == (None, None, S.Done)
    it, err = S.NewSuperSSTableReader(sr.readers, comp=lambda a, b: (a < b) - (a > b)).Scan()
    assert it is None and isinstance(err, S.UnsupportedError) and "BytesComparator" in str(err)
    sr._free_stack()


def test_bounds_equal_bisect(tmp_path):
    import bisect

    tables = scan_tables()
    sr = open_stack(tmp_path, tables)
    sr.GetBatch([b"x"])  # builds the stack
    qs = [b"", b"\0", be(0), be(1), be(39), be(40), be(50), be(51), P8, P8 + b"a", P8 + b"c", P8 + b"cc", P8 + b"i", b"k" * 1500,
          b"\xff"]
    d_keys, d_off, nbytes = arena(qs)
    T = len(tables)
    for upper in (0, 1):
        pos = torch.full((len(qs) * T,), -1, dtype=torch.int64, device="cuda")
        assert L.lib().rio_sst_stack_bounds(sr._stack, d_keys.data_ptr(), d_off.data_ptr(), len(qs), nbytes, upper,
                                            pos.data_ptr(), None) == L.RIO_OK
        torch.cuda.synchronize()
        fn = bisect.bisect_right if upper else bisect.bisect_left
        assert pos.cpu().tolist() == [fn(sorted(t), q) for q in qs for t in tables]
    sr._free_stack()


def test_keys_gather_needs_a_plan():
    lib = L.lib()
    h = ctypes.c_void_p()
    assert lib.rio_ctx_create(0, ctypes.byref(h)) == L.RIO_OK
    try:
        buf = torch.zeros(8, dtype=torch.int64, device="cuda")
        assert lib.rio_sst_keys_gather(h, buf.data_ptr(), 2, buf.data_ptr(), 64, buf.data_ptr(), None) == L.RIO_ERR_STATE
        assert lib.rio_sst_keys_gather(h, buf.data_ptr(), 0, buf.data_ptr(), 64, buf.data_ptr(), None) == L.RIO_ERR_STATE
    finally:
        lib.rio_ctx_destroy(h)


# ---- capture, lifetime, metadata -----------------------------------------------------------------------------------

def test_lookup_plan_and_copy_replay_from_one_graph(tmp_path):
    tables = [{be(i): b"old-%d" % i for i in range(0, 64)}, {be(i): None if i % 5 == 0 else val(i, i) for i in range(0, 64, 2)}]
    sr = open_stack(tmp_path, tables)
    model = sm.Stack(tables)
    n = 48
    first, second = [be(i) for i in range(n)], [be(i) for i in range(80, 80 - n, -1)]
    sr.GetBatch(first[:2])  # the stack exists before the capture: nothing is created inside it
    d_keys, d_off, nbytes = arena(first)
    src = torch.zeros(n, dtype=torch.int64, device="cuda")
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    val_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    cap = 4096
    values = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    lib = L.lib()
    g = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=stream):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.rio_sst_stack_lookup(sr._stack, 0, d_keys.data_ptr(), d_off.data_ptr(), n, nbytes, src.data_ptr(), st) == 0
        assert lib.rio_sst_stack_value_plan(sr._stack, src.data_ptr(), n, 1, status.data_ptr(), val_off.data_ptr(), st) == 0
        assert lib.rio_sst_stack_value_copy(sr._stack, src.data_ptr(), n, val_off.data_ptr(), values.data_ptr(), cap, st) == 0
    for queries in (first, second):
        d_keys.copy_(arena(queries)[0])  # same buffers, other contents (every key is four bytes)
        g.replay()
        torch.cuda.synchronize()
        want = [model.get(q) for q in queries]
        vals = [v for v in want if v is not sm.NOT_FOUND and v is not None]
        off = val_off.cpu().tolist()
        assert off[n] == sum(len(v) for v in vals) <= cap
        assert bytes(values[:off[n]].cpu().numpy()) == b"".join(vals)
        assert status.cpu().tolist() == [L.RIO_GET_NOT_FOUND if v is sm.NOT_FOUND else L.RIO_GET_NIL if v is None
                                         else L.RIO_GET_VALUE for v in want]
    assert any(v is sm.NOT_FOUND for v in want) and any(v is None for v in want)
    sr._free_stack()


def test_close_then_a_batched_call_is_an_error(tmp_path):
    tables = [{be(1): b"one"}, {be(2): b"two"}]
    sr = open_stack(tmp_path, tables)
    assert sr.GetBatch([be(1), be(3)]) == [(b"one", None), (None, S.NotFound)]
    assert sr._stack is not None
    assert sr.Close() is None and sr._stack is None
    assert sr.Close() is None  # the stack is freed once
    sr._free_stack()
    for got in (sr.GetBatch([be(1)]), sr.ContainsBatch([be(1)])):
        assert len(got) == 1 and isinstance(got[0][1], S.UnsupportedError)
    it, err = sr.Scan()
    assert it is None and isinstance(err, S.UnsupportedError)


def test_metadata_and_base_path(tmp_path):
    tables = [{be(5): b"x", be(9): b"y"}, {be(1): b"z" * 50, be(7): None, be(8): b""}, {be(3): b"w"}]
    sr = open_stack(tmp_path, tables)
    metas = [r.MetaData() for r in sr.readers]
    want = sm.metadata([(m.numRecords, m.dataBytes, m.indexBytes, m.totalBytes, m.version, m.minKey, m.maxKey) for m in metas])
    m = sr.MetaData()
    assert (m.numRecords, m.dataBytes, m.indexBytes, m.totalBytes, m.version, m.minKey, m.maxKey) == want
    assert (m.numRecords, m.version, m.minKey, m.maxKey) == (6, 1, be(5), be(9))  # MinKey: the largest first key
    assert sr.BasePath() == ",".join(str(tmp_path / f"t{i}") for i in range(3))
    assert sr.Close() is None
