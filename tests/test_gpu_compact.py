"""Merge-compaction on the device (GPU): NewSSTableMerger().Merge / MergeCompact over loaded tables
against a plain Python model of sstables/sstable_merger.go written out by the host writer. All three
output files must be byte-identical to the model's table; the device output is then reopened with
NewSSTableReader (validation on) and its scan compared with the model's pairs."""
import os
import random
import struct

import pytest

import compact_model as M
import sstables as S
from recordio import _lib as L
from sstables import proto
from sstables.writer import _Image, crc64_iso, write_sstable

pytestmark = pytest.mark.gpu

FILES = ("data.rio", "index.rio", "meta.pb.bin")
ALL, LATEST, SKIP = "all", S.ScanReduceLatestWins, S.ScanReduceLatestWinsSkipTombstones
MODEL_REDUCE = {LATEST: M.reduce_latest_wins, SKIP: M.reduce_latest_wins_skip_tombstones}


def be(i):
    return struct.pack(">I", i)


def scan_all(r):
    it, err = r.Scan()
    assert err is None
    out = []
    while True:
        k, v, err = it.Next()
        if err is S.Done:
            return out
        assert err is None, err
        out.append((k, v))


def open_tables(tmp_path, tables, in_comp=2):
    readers = []
    for t, items in enumerate(tables):
        base = str(tmp_path / f"in{t}")
        write_sstable(base, items, in_comp)
        r, err = S.NewSSTableReader(S.ReadBasePath(base))
        assert err is None, err
        readers.append(r)
    return readers


def model_pairs(tables, mode):
    return M.merge_all(tables) if mode == ALL else M.merge_compact(tables, MODEL_REDUCE[mode])


def run_merge(readers, out, mode, out_comp=None):
    m = S.NewSSTableMerger()
    kw = {} if out_comp is None else {"data_compression": out_comp}
    return m.Merge(readers, out, **kw) if mode == ALL else m.MergeCompact(readers, out, mode, **kw)


def check(tmp_path, tables, mode, in_comp=2, out_comp=None):
    """Device output == the model's table in all three files, and scans back as the model's pairs."""
    pairs = model_pairs(tables, mode)
    want, got = str(tmp_path / "want"), str(tmp_path / "got")
    want_meta = write_sstable(want, pairs, 2 if out_comp is None else out_comp)
    readers = open_tables(tmp_path, tables, in_comp)
    err = run_merge(readers, got, mode, out_comp)
    assert err is None, err
    for name in FILES:
        a, b = open(os.path.join(got, name), "rb").read(), open(os.path.join(want, name), "rb").read()
        assert len(a) == len(b), (name, len(a), len(b))
        assert a == b, name
    r, err = S.NewSSTableReader(S.ReadBasePath(got))
    assert err is None, err
    assert scan_all(r) == pairs
    assert r.MetaData().numRecords == len(pairs) == want_meta.numRecords
    return pairs, r.MetaData()


# ---- the reference's shapes (sstable_merger_test.go) ------------------------------------------------

@pytest.mark.parametrize("n_tables", [1, 2, 3, 4, 5])
def test_identical_tables_of_ascending_integers(tmp_path, n_tables):
    """writeMergeCompactAndCheck (:60-117): every table holds the same 200 keys; the last one's values win."""
    tables = [[(be(i), be(i) + bytes([t])) for i in range(200)] for t in range(n_tables)]
    pairs, _ = check(tmp_path, tables, LATEST)
    assert pairs == tables[-1]


def test_five_overlapping_tables(tmp_path):
    """TestOverlappingMergeAndCompact (:119-161): table i holds 250 keys from i * 25 on."""
    tables = [[(be(k), be(k * 7 + t)) for k in range(t * 25, t * 25 + 250)] for t in range(5)]
    pairs, meta = check(tmp_path, tables, LATEST)
    assert [k for k, _ in pairs] == [be(k) for k in range(350)]
    assert (meta.minKey, meta.maxKey) == (be(0), be(349))


def test_all_tombstones_give_an_empty_table(tmp_path):
    """TestMergeAndCompactEmptyResult (:163-195): every group reduces to nothing."""
    tables = [[(be(k), b"") for k in range(t * 25, t * 25 + 250)] for t in range(5)]
    pairs, meta = check(tmp_path, tables, SKIP)
    assert pairs == [] and meta.numRecords == 0 and meta.minKey == b"" and meta.maxKey == b""


# ---- key ordering -----------------------------------------------------------------------------------

def _ordering_tables():
    p8, p9, p16 = b"prefix_8", b"prefix_9x", b"sixteen_byte_pfx"
    keys = [b"a", b"a\0", b"a\0\0", b"ab", b"\x7f", b"\x80", b"\x80\x00", b"\xff", b"\xff\xff", b"\x7f\xff\x80",
            p8, p8 + b"\0", p8 + b"\x01", p8 + b"\x80", p9 + b"a", p9 + b"b", p9 + b"\xfe", p16, p16 + b"\0",
            p16 + b"a", p16 + b"\xff", p16 + b"aa"]
    keys += [bytes([0x61 + (n % 3)]) * n for n in range(1, 41)]       # lengths 1 .. 40
    keys += [b"\xc3" * n + b"\x80" for n in range(1, 41)]
    keys = sorted(set(keys))
    rng = random.Random(5)
    tables = [[], [], [], []]
    for k in keys:  # every key in one to three tables, chosen so that equal prefixes meet across tables
        for t in rng.sample(range(4), rng.randint(1, 3)):
            tables[t].append((k, b"v%d:" % t + k[:5]))
    return tables


@pytest.mark.parametrize("mode", [LATEST, SKIP])
def test_key_ordering_prefixes_and_high_bytes(tmp_path, mode):
    tables = _ordering_tables()
    pairs, _ = check(tmp_path, tables, mode)
    assert [k for k, _ in pairs] == sorted({k for t in tables for k, _ in t})


def test_key_ordering_under_merge_with_disjoint_tables(tmp_path):
    keys = sorted({k for t in _ordering_tables() for k, _ in t})
    tables = [[(k, b"x" + k) for k in keys[t::3]] for t in range(3)]
    pairs, _ = check(tmp_path, tables, ALL)
    assert [k for k, _ in pairs] == keys


# ---- values: nil, empty and non-empty winners and losers --------------------------------------------

_KINDS = (None, b"", b"value")


def _value_tables():
    """Three tables; each key has kind w in the highest table that holds it and kind lo in every table
    below that one, and the highest table is each of the three in turn."""
    tables = [[], [], []]
    n = 0
    for w in _KINDS:
        for lo in _KINDS:
            for top in (0, 1, 2):  # the highest table holding the key
                k = b"key%03d" % n
                n += 1
                tables[top].append((k, w if w is None or w == b"" else w + bytes([top])))
                for below in range(top):
                    tables[below].append((k, lo if lo is None or lo == b"" else lo + bytes([below])))
    return tables


@pytest.mark.parametrize("mode", [LATEST, SKIP])
def test_nil_empty_and_non_empty_winners_and_losers(tmp_path, mode):
    pairs, meta = check(tmp_path, _value_tables(), mode)
    assert meta.nullValues == 0  # a nil winner drops its group
    kinds = {b"" if v == b"" else b"x" for _, v in pairs}
    assert kinds == ({b"", b"x"} if mode is LATEST else {b"x"})


def test_merge_keeps_nil_values(tmp_path):
    tables = [[(bytes([0x41 + t]) + k, v) for k, v in items] for t, items in enumerate(_value_tables())]
    pairs, meta = check(tmp_path, tables, ALL)
    nils = sum(v is None for _, v in pairs)
    assert nils > 0 and meta.nullValues == nils
    assert len(pairs) == sum(len(t) for t in tables)


# ---- value lengths and alignment --------------------------------------------------------------------

_LENS = (0, 1, 15, 16, 17, 63, 64, 65, 255, 1023, 1024, 1025, 4096, 70000)


@pytest.mark.parametrize("in_comp,out_comp", [(0, 0), (0, 2), (2, 0), (2, 2)])
def test_value_lengths_and_misalignment(tmp_path, in_comp, out_comp):
    """Every length class of the gather (lane group / wave, head / body / tail) at source and
    destination offsets that differ: the two tables hold the lengths in different orders with a
    3- and a 5-byte value between them, and the merge interleaves them."""
    rng = random.Random(9)
    val = lambda n: rng.randbytes(n // 2) + bytes(n - n // 2)  # noqa: E731  (half random, half compressible)
    a, b = [], []
    for j, n in enumerate(_LENS):
        a += [(b"k%02d-a" % j, val(n)), (b"k%02d-c" % j, val(3))]
    for j, n in enumerate(_LENS[::-1] + _LENS[3:7]):
        b += [(b"k%02d-b" % j, val(n)), (b"k%02d-d" % j, val(5))]
    check(tmp_path / "compact", [a, b], LATEST, in_comp, out_comp)
    check(tmp_path / "merge", [a, b], ALL, in_comp, out_comp)


# ---- table shapes -----------------------------------------------------------------------------------

def test_an_empty_table_among_the_inputs(tmp_path):
    tables = [[(be(i), be(i)) for i in range(0, 300, 2)], [], [(be(i), b"n%d" % i) for i in range(0, 300, 3)]]
    check(tmp_path, tables, LATEST)


@pytest.mark.parametrize("mode", [ALL, LATEST])
def test_all_tables_empty(tmp_path, mode):
    pairs, meta = check(tmp_path, [[], [], []], mode)
    assert pairs == [] and meta.numRecords == 0


@pytest.mark.parametrize("one_first", [True, False])
def test_one_entry_against_five_thousand(tmp_path, one_first):
    big = [(be(i), be(i ^ 0x5A5A)) for i in range(5000)]
    one = [(be(2500), b"the one")]
    pairs, _ = check(tmp_path, [one, big] if one_first else [big, one], LATEST)
    assert len(pairs) == 5000 and (pairs[2500][1] == b"the one") == (not one_first)


def test_sixteen_tables(tmp_path):
    rng = random.Random(16)
    tables = [sorted((be(k), b"t%02d-%d" % (t, k)) for k in rng.sample(range(1500), 400)) for t in range(16)]
    check(tmp_path, tables, LATEST)


# ---- randomised -------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,mode", [(1, LATEST), (2, SKIP)])
def test_randomised_eight_tables(tmp_path, seed, mode):
    rng = random.Random(seed)
    universe = sorted({rng.randbytes(rng.randint(1, 24)) for _ in range(12000)})
    tables = []
    for t in range(8):
        items = []
        for k in sorted(rng.sample(universe, 3000 + rng.randint(-200, 200))):
            r = rng.random()
            items.append((k, None if r < 0.1 else b"" if r < 0.2 else rng.randbytes(rng.randint(1, 48))))
        tables.append(items)
    pairs, _ = check(tmp_path, tables, mode)
    assert 0 < len(pairs) < sum(len(t) for t in tables)


# ---- errors -----------------------------------------------------------------------------------------

def test_merge_with_a_duplicate_key_writes_nothing(tmp_path):
    tables = [[(be(i), be(i)) for i in range(0, 100, 2)], [(be(i), be(i)) for i in range(1, 100, 2)] + [(be(100), b"")],
              [(be(58), b"again")]]
    readers = open_tables(tmp_path, tables)
    out = str(tmp_path / "out")
    err = run_merge(readers, out, ALL)
    assert str(err) == f"sstables.WriteNext '{out}': the same key cannot be written more than once"
    assert not isinstance(err, S.UnsupportedError)
    assert not os.path.exists(out)
    assert run_merge(readers[:2], out, ALL) is None  # without the duplicate the same readers merge
    assert sorted(os.listdir(out)) == sorted(FILES)


def _table_with_index(base, items, index_keys, comp=2):
    """data.rio as the writer makes it for `items`; index.rio rebuilt by hand with `index_keys` in place
    of the items' keys (offsets and checksums stay the writer's)."""
    write_sstable(base, items, comp)
    d, ix = _Image(comp), _Image(0)
    for (_, v), k in zip(items, index_keys):
        ix.write(proto.encode_index_entry(k, d.write(v), crc64_iso(v or b"")))
    with open(os.path.join(base, "index.rio"), "wb") as fh:
        fh.write(ix.bytes())


@pytest.mark.parametrize("shape", ["swapped", "repeated", "last"])
@pytest.mark.parametrize("mode", [ALL, LATEST])
def test_unsorted_input_is_refused(tmp_path, shape, mode):
    """The plan checks each table's order: one key out of place gives UnsupportedError and no output."""
    items = [(be(i * 3), be(i)) for i in range(600)]
    keys = [k for k, _ in items]
    if shape == "swapped":
        keys[300], keys[301] = keys[301], keys[300]
    elif shape == "repeated":
        keys[17] = keys[16]
    else:
        keys[-1] = be(1)
    good = str(tmp_path / "good")
    write_sstable(good, [(be(i * 3 + 1), b"g") for i in range(700)])
    bad = str(tmp_path / "bad")
    _table_with_index(bad, items, keys)
    readers = []
    for base in (good, bad):
        r, err = S.NewSSTableReader(S.ReadBasePath(base))
        assert err is None, err
        readers.append(r)
    out = str(tmp_path / "out")
    err = run_merge(readers, out, mode)
    assert isinstance(err, S.UnsupportedError), err
    assert "bad" in str(err) and not os.path.exists(out)


def test_value_failing_its_stored_checksum(tmp_path):
    """A table opened with SkipHashCheckOnLoad whose entry 7 stores a wrong checksum: refused when the reader
    checks hashes on reads; otherwise merged as the reference merges it, the new index carrying the CRC-64
    of the value as read (the model's table, which the host writer hashes itself)."""
    items = [(be(i), b"value-%d" % i) for i in range(40)]
    other = [(be(i), b"other-%d" % i) for i in range(20, 60)]
    bad, good = str(tmp_path / "bad"), str(tmp_path / "good")
    write_sstable(good, other)
    write_sstable(bad, items)
    d, ix = _Image(2), _Image(0)
    for j, (k, v) in enumerate(items):
        ix.write(proto.encode_index_entry(k, d.write(v), crc64_iso(v) ^ (j == 7)))
    with open(os.path.join(bad, "index.rio"), "wb") as fh:
        fh.write(ix.bytes())
    out = str(tmp_path / "out")
    g, err = S.NewSSTableReader(S.ReadBasePath(good))
    assert err is None
    r, err = S.NewSSTableReader(S.ReadBasePath(bad), S.SkipHashCheckOnLoad(), S.EnableHashCheckOnReads())
    assert err is None
    assert isinstance(run_merge([r, g], out, LATEST), S.UnsupportedError) and not os.path.exists(out)
    r, err = S.NewSSTableReader(S.ReadBasePath(bad), S.SkipHashCheckOnLoad())
    assert err is None
    assert run_merge([r, g], out, LATEST) is None
    want = str(tmp_path / "want")
    write_sstable(want, M.merge_compact([items, other], M.reduce_latest_wins))
    for name in FILES:
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(want, name), "rb").read(), name


def test_refused_arguments(tmp_path):
    readers = open_tables(tmp_path, [[(b"a", b"1")], [(b"a", b"2")]])
    m, out = S.NewSSTableMerger(), str(tmp_path / "out")
    err = m.MergeCompact(readers, out, lambda k, vs, cs: (k, vs[0]))
    assert isinstance(err, S.UnsupportedError)
    err = m.MergeCompact(readers, out, M.reduce_latest_wins)  # the model's function is not the exported object
    assert isinstance(err, S.UnsupportedError)
    # a v0 table: no meta.pb.bin, values are DataEntry protos
    v0 = str(tmp_path / "v0")
    write_sstable(v0, [(b"a", b"\x0a\x01x")])
    os.remove(os.path.join(v0, "meta.pb.bin"))
    r0, err = S.NewSSTableReader(S.ReadBasePath(v0))
    assert err is None and r0.MetaData().version == 0
    for call in (lambda: m.MergeCompact([readers[0], r0], out, LATEST), lambda: m.Merge([r0], out)):
        assert isinstance(call(), S.UnsupportedError)
    assert isinstance(m.Merge([], out), S.UnsupportedError)
    assert isinstance(m.Merge(readers[:1], out, data_compression=L.COMP_GZIP), S.UnsupportedError)
    assert not os.path.exists(out)
