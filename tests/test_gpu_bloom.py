"""Bloom filters and point lookups on the device (GPU): rio_bloom_add / rio_sst_bloom_add / rio_bloom_contains /
rio_sst_key_prefixes / rio_sst_lookup (csrc/rio_bloom.hip) against the model of tests/bloom_model.py and
bisect on the host, then the mirror end to end. Bits are compared word for word with the model given the same
hash keys, hits entry for entry (false positives included)."""
import bisect
import ctypes
import os
import random
import shutil
import struct

import numpy as np
import pytest
import torch

import bloom_model as bm
import memstore as MS
import simpledb as DB
import sstables as S
from conftest import GOLDEN
from recordio import _lib as L
from sstables import bloom
from sstables.merger import table_view
from sstables.writer import write_sstable

pytestmark = pytest.mark.gpu

_NONE = 0xFFFFFFFFFFFFFFFF
FILES3 = ["data.rio", "index.rio", "meta.pb.bin"]
FILES4 = ["bloom.bf.gz"] + FILES3
GRID_CAP, BLOCK = 2048, 256  # kBloomGridCap blocks of 256 lanes (rio_bloom.hip)


def be(i):
    return struct.pack(">I", i)


def hash_keys(k, seed):
    rng = random.Random(seed)
    return [rng.getrandbits(64) for _ in range(k)]


def up(a, dt):
    return torch.from_numpy(np.array(a, dtype=dt)).cuda()  # a writable copy


class Arena:
    """Keys back to back from byte `lead` on; the last key ends exactly at the arena's (and the tensor's) end."""

    def __init__(self, keys, lead=0):
        self.keys = [bytes(k) for k in keys]
        raw = b"\xEE" * lead + b"".join(self.keys)
        self.nbytes = len(raw)
        self.d_keys = up(np.frombuffer(raw or b"\0", dtype=np.uint8), np.uint8)
        self.d_off = up(lead + np.cumsum([0] + [len(k) for k in self.keys]), np.int64)
        self.n = len(self.keys)


class DevFilter:
    def __init__(self, m, hk, words=None):
        self.m, self.hk = m, list(hk)
        nw = (m + 63) // 64
        self.bits = torch.zeros(nw, dtype=torch.int64, device="cuda") if words is None else up(
            np.asarray(words, dtype=np.uint64).view(np.int64), np.int64)
        self.keys = up(np.asarray(self.hk, dtype=np.uint64).view(np.int64), np.int64)
        self.view = L.BloomView(bits=self.bits.data_ptr(), hash_keys=self.keys.data_ptr(), m=m, k=len(self.hk))

    def ref(self):
        return ctypes.byref(self.view)

    def words(self):
        torch.cuda.synchronize()
        return self.bits.cpu().numpy().view(np.uint64)


def ctx():
    return L.default_ctx(0)


def dev_add(f, a, stream=None):
    rc = L.lib().rio_bloom_add(ctx(), f.ref(), a.d_keys.data_ptr(), a.d_off.data_ptr(), a.n, a.nbytes, stream)
    assert rc == L.RIO_OK, L.strerror(rc)


def dev_contains(f, a, stream=None, hit=None):
    hit = torch.full((max(a.n, 1),), 0xAA, dtype=torch.uint8, device="cuda") if hit is None else hit
    rc = L.lib().rio_bloom_contains(ctx(), f.ref(), a.d_keys.data_ptr(), a.d_off.data_ptr(), a.n, a.nbytes,
                                    hit.data_ptr(), stream)
    assert rc == L.RIO_OK, L.strerror(rc)
    torch.cuda.synchronize()
    return hit[:a.n].cpu().tolist()


def model_of(m, hk, keys):
    f = bm.Model(m, hk)
    for k in keys:
        f.add(k)
    return f


def assert_words(f, model):
    np.testing.assert_array_equal(f.words(), np.asarray(model.words, dtype=np.uint64))


# ---- the hash: key lengths and alignments ------------------------------------------------------------------------

LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 1024)


@pytest.mark.parametrize("lead", range(8))
def test_key_lengths_at_every_arena_offset(lead):
    """Every length with its first byte at arena offset `lead` (the tensors are 256-byte aligned, so this is the
    address alignment too) and its last byte the arena's last; then all of them back to back in one arena."""
    rng = random.Random(100 + lead)
    hk = hash_keys(7, lead)
    f = DevFilter(9586, hk)
    keys = []
    for n in LENGTHS:
        key = rng.randbytes(n)
        a = Arena([key], lead)
        assert a.d_keys.data_ptr() % 256 == 0 and int(a.d_off[0].item()) == lead
        assert int(a.d_off[-1].item()) == a.nbytes and a.d_keys.numel() == max(a.nbytes, 1)
        dev_add(f, a)  # adds compose
        keys.append(key)
        assert dev_contains(f, a) == [1]
    assert_words(f, model_of(9586, hk, keys))
    together = [rng.randbytes(n) for n in LENGTHS + LENGTHS[::-1]]
    a = Arena(together, lead)
    assert int(a.d_off[-1].item()) == a.nbytes == a.d_keys.numel()
    g = DevFilter(9586, hk)
    dev_add(g, a)
    assert_words(g, model_of(9586, hk, together))
    assert dev_contains(g, a) == [1] * a.n


@pytest.mark.parametrize("m", [2, 64, 9586])
@pytest.mark.parametrize("k", [1, 7, 30, 64])
def test_filter_shapes(m, k):
    rng = random.Random(m * 100 + k)
    keys = [rng.randbytes(rng.randint(0, 20)) for _ in range(40)]
    hk = hash_keys(k, m + k)
    f = DevFilter(m, hk)
    dev_add(f, Arena(keys))
    model = model_of(m, hk, keys)
    assert_words(f, model)
    probe = Arena([rng.randbytes(rng.randint(0, 20)) for _ in range(300)] + keys[:5], lead=3)
    assert dev_contains(f, probe) == [int(model.contains(q)) for q in probe.keys]


def test_contention_every_lane_on_three_dwords():
    keys = [be(i) for i in range(10_000)]
    hk = hash_keys(7, 96)
    f = DevFilter(96, hk)
    dev_add(f, Arena(keys))
    assert_words(f, model_of(96, hk, keys))


# ---- launch shapes ---------------------------------------------------------------------------------------------

def test_no_keys_and_one_key():
    hk = hash_keys(7, 1)
    f = DevFilter(9586, hk)
    dev_add(f, Arena([]))
    assert not f.words().any()
    assert dev_contains(f, Arena([])) == []
    dev_add(f, Arena([b"only"]))
    assert_words(f, model_of(9586, hk, [b"only"]))
    assert dev_contains(f, Arena([b"only", b"other"])) == [1, int(model_of(9586, hk, [b"only"]).contains(b"other"))]


def test_more_keys_than_one_round_of_the_grid():
    n = GRID_CAP * BLOCK + 1
    rows = np.arange(n, dtype=">u4").view(np.uint8).reshape(n, 4)
    a = Arena([])
    a.d_keys, a.d_off, a.n, a.nbytes = up(rows.reshape(-1), np.uint8), up(4 * np.arange(n + 1), np.int64), n, 4 * n
    m, k = bm.optimal(n, 0.01)
    hk = hash_keys(k, 5)
    f = DevFilter(m, hk)
    dev_add(f, a)
    want = bm.words_fixed_np(m, hk, rows)
    np.testing.assert_array_equal(f.words(), want)
    # key n - 1 is the one the second round of the grid-stride loop handles: without it the words differ
    assert not np.array_equal(want, bm.words_fixed_np(m, hk, rows[:-1]))
    hit = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dev_contains(f, a, hit=hit)
    assert int(hit.sum().item()) == n


def test_m_past_32_bits():
    """m = 2^32 + 9: where a 32-bit modulo or word index goes wrong. 512 MiB of zero-filled bits; the non-zero
    words are found on the device and compared with the model's, position and value."""
    m = (1 << 32) + 9
    keys = [be(i) + b"-wide" for i in range(64)]
    hk = hash_keys(7, 32)
    f = DevFilter(m, hk)
    assert f.bits.numel() * 8 == 512 * 1024 * 1024 + 8
    dev_add(f, Arena(keys))
    torch.cuda.synchronize()
    nz = torch.nonzero(f.bits).flatten()
    got = {int(i): int(w) & _NONE for i, w in zip(nz.cpu().tolist(), f.bits[nz].cpu().tolist())}
    want = bm.sparse_words(m, hk, keys)
    assert sum(bin(w).count("1") for w in got.values()) == sum(bin(w).count("1") for w in want.values())
    assert got == want
    probe = Arena(keys + [be(i) + b"-none" for i in range(64)])
    model_hits = [int(all((want.get(i >> 6, 0) >> (i & 63)) & 1 for i in
                          [(bm.fnv1_64(q) ^ h) % m for h in hk])) for q in probe.keys]
    assert model_hits[:64] == [1] * 64
    assert dev_contains(f, probe) == model_hits
    # a modulo taken in 32 bits would have set other bits: at least one probe's index differs between the two
    assert any(((bm.fnv1_64(q) ^ h) % m) != (((bm.fnv1_64(q) ^ h) & 0xFFFFFFFF) % (m & 0xFFFFFFFF)) for q in keys for h in hk)


def test_two_adds_compose():
    rng = random.Random(8)
    keys = [rng.randbytes(rng.randint(1, 40)) for _ in range(500)]
    hk = hash_keys(7, 8)
    one, two = DevFilter(9586, hk), DevFilter(9586, hk)
    dev_add(one, Arena(keys))
    dev_add(two, Arena(keys[:200], lead=1))
    dev_add(two, Arena(keys[200:], lead=5))
    np.testing.assert_array_equal(one.words(), two.words())
    assert_words(one, model_of(9586, hk, keys))


def test_a_callers_stream():
    rng = random.Random(9)
    keys = [rng.randbytes(12) for _ in range(1000)]
    hk = hash_keys(7, 9)
    a, f = Arena(keys), DevFilter(9586, hk)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=0)
    st = ctypes.c_void_p(s.cuda_stream)
    hit = torch.zeros(len(keys), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dev_add(f, a, stream=st)
    assert dev_contains(f, a, stream=st, hit=hit) == [1] * len(keys)  # ordered after the add on the same stream
    s.synchronize()
    assert_words(f, model_of(9586, hk, keys))


def test_graph_capture_and_replay_of_add_and_contains():
    rng = random.Random(10)
    keys = [rng.randbytes(rng.randint(0, 30)) for _ in range(3000)]
    absent = [rng.randbytes(31) for _ in range(3000)]
    hk = hash_keys(7, 10)
    a, q, f = Arena(keys), Arena(keys + absent), DevFilter(9586, hk)
    hit = torch.zeros(q.n, dtype=torch.uint8, device="cuda")
    lib = L.lib()

    def launch(st):
        assert lib.rio_bloom_add(ctx(), f.ref(), a.d_keys.data_ptr(), a.d_off.data_ptr(), a.n, a.nbytes, st) == L.RIO_OK
        assert lib.rio_bloom_contains(ctx(), f.ref(), q.d_keys.data_ptr(), q.d_off.data_ptr(), q.n, q.nbytes,
                                      hit.data_ptr(), st) == L.RIO_OK

    s = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    st = ctypes.c_void_p(s.cuda_stream)
    launch(st)  # one launch on the capture stream first, as the decode's graph test does
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launch(st)
    model = model_of(9586, hk, keys)
    want = [int(model.contains(x)) for x in q.keys]
    for _ in range(2):
        f.bits.zero_()
        hit.fill_(0xAA)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        assert_words(f, model)
        assert hit.cpu().tolist() == want


def test_contains_with_false_positives_and_misses():
    rng = random.Random(11)
    keys = [rng.randbytes(rng.randint(0, 24)) for _ in range(2000)]
    m, k = bm.optimal(2000, 0.05)
    hk = hash_keys(k, 11)
    model = model_of(m, hk, keys)
    absent = [b"absent/" + be(i) for i in range(4000)]
    absent = [x for x in absent if x not in set(keys)]
    want = [model.contains(x) for x in absent]
    assert any(want) and not all(want)  # the model itself reports a false positive and a miss
    f = DevFilter(m, hk, model.words)  # the model's bits, uploaded
    assert dev_contains(f, Arena(keys, lead=2)) == [1] * len(keys)
    assert dev_contains(f, Arena(absent, lead=7)) == [int(x) for x in want]
    built = DevFilter(m, hk)
    dev_add(built, Arena(keys))
    assert_words(built, model)
    assert dev_contains(built, Arena(absent)) == [int(x) for x in want]


# ---- rio_sst_lookup --------------------------------------------------------------------------------------------

def open_table(base, items, *opts):
    write_sstable(base, items)
    r, err = S.NewSSTableReader(S.ReadBasePath(base), *opts)
    assert err is None, err
    return r


def dev_lookup(r, queries, f=None, lead=0):
    lib = L.lib()
    view = table_view(r.t)
    pfx = torch.full((max(r.t.n_index, 1),), -1, dtype=torch.int64, device="cuda")
    assert lib.rio_sst_key_prefixes(ctx(), ctypes.byref(view), pfx.data_ptr(), None) == L.RIO_OK
    q = Arena(queries, lead)
    out = torch.full((max(q.n, 1),), 0x55, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc = lib.rio_sst_lookup(ctx(), ctypes.byref(view), pfx.data_ptr(), f.ref() if f is not None else None,
                            q.d_keys.data_ptr(), q.d_off.data_ptr(), q.n, q.nbytes, out.data_ptr(), None)
    assert rc == L.RIO_OK, L.strerror(rc)
    torch.cuda.synchronize()
    want_pfx = [int.from_bytes(k[:8].ljust(8, b"\0"), "big") for k in (r.t.key(i) for i in range(r.t.n_index))]
    assert [x & _NONE for x in pfx[:r.t.n_index].cpu().tolist()] == want_pfx
    return [x & _NONE for x in out[:q.n].cpu().tolist()]


def host_lookup(keys, queries):
    out = []
    for q in queries:
        i = bisect.bisect_left(keys, q)
        out.append(i if i < len(keys) and keys[i] == q else _NONE)
    return out


def _lookup_keys():
    p8, p16 = b"prefix_8", b"sixteen_byte_pfx"
    keys = [b"a", b"a\0", b"a\0\0", b"ab", b"\x7f", b"\x80", b"\x80\x00", b"\xff\xff", p8, p8 + b"\0", p8 + b"\x01",
            p8 + b"\x80", p8 + b"tail-a", p8 + b"tail-b", p16, p16 + b"\0", p16 + b"a", p16 + b"\xff"]
    keys += [be(i) for i in range(10, 2000, 3)]
    keys += [b"k" * n for n in range(1, 41)]
    return sorted(set(keys))


def _queries(keys):
    qs = [b"", b"\0", b"\xff\xff\xff", b"a", b"a\0", b"a\0\0\0", b"aa", b"prefix_", b"prefix_8", b"prefix_8tail-",
          b"prefix_8tail-c", b"prefix_8tail-a", b"sixteen_byte_pf", b"sixteen_byte_pfxa", b"sixteen_byte_pfxb"]
    qs += [be(i) for i in range(0, 2010)]                 # below the first, between neighbours, present, above the last
    qs += [k + b"\0" for k in keys[:60]] + [k[:-1] for k in keys[:60]]
    return qs + list(keys)


@pytest.mark.parametrize("with_empty_key", [False, True])
def test_lookup_equals_bisect(tmp_path, with_empty_key):
    keys = _lookup_keys()
    if with_empty_key:
        keys = [b""] + keys
    r = open_table(str(tmp_path / "t"), [(k, b"v" + k[:3]) for k in keys])
    qs = _queries(keys)
    want = host_lookup(keys, qs)
    assert _NONE in want and any(w != _NONE for w in want)
    assert want[qs.index(b"")] == (0 if with_empty_key else _NONE)
    assert want[qs.index(b"a")] != _NONE and want[qs.index(b"a\0")] == want[qs.index(b"a")] + 1
    for lead in (0, 3):
        assert dev_lookup(r, qs, lead=lead) == want
    # a filter built from the table's keys changes nothing; an all-zero filter rejects every query
    m, k = bm.optimal(len(keys), 0.01)
    hk = hash_keys(k, 12)
    model = model_of(m, hk, keys)
    assert dev_lookup(r, qs, f=DevFilter(m, hk, model.words)) == want
    assert dev_lookup(r, qs, f=DevFilter(m, hk)) == [_NONE] * len(qs)
    # a filter holding half of the keys: exactly the queries it rejects turn into ~0
    half = model_of(m, hk, keys[::2])
    assert dev_lookup(r, qs, f=DevFilter(m, hk, half.words)) == [w if half.contains(q) else _NONE for q, w in zip(qs, want)]


@pytest.mark.parametrize("n", [0, 1])
def test_lookup_in_tables_of_no_and_one_entry(tmp_path, n):
    keys = [b"single"][:n]
    r = open_table(str(tmp_path / "t"), [(k, b"v") for k in keys])
    qs = [b"", b"a", b"single", b"singl", b"single\0", b"z"]
    assert dev_lookup(r, qs) == host_lookup(keys, qs)
    assert dev_lookup(r, []) == []


# ---- the mirror, end to end ------------------------------------------------------------------------------------

def _same(batch, loop):
    assert len(batch) == len(loop)
    for (bv, be_), (lv, le) in zip(batch, loop):
        assert bv == lv and type(bv) is type(lv)
        assert (be_ is None) == (le is None) and str(be_) == str(le)
        assert (be_ is S.NotFound) == (le is S.NotFound)  # the sentinel stays the sentinel


def _golden_with_filter(tmp_path, table_dir, table, fixture):
    base = str(tmp_path / fixture.replace("/", "_"))
    shutil.copytree(os.path.join(GOLDEN, table_dir, table), base)
    shutil.copy(os.path.join(GOLDEN, "bloom", fixture, "bloom.bf.gz"), os.path.join(base, "bloom.bf.gz"))
    return base


@pytest.mark.parametrize("check_reads", [False, True])
def test_batches_equal_loops(tmp_path, check_reads):
    opts = (S.EnableHashCheckOnReads(),) if check_reads else ()
    items = [(be(1), b"one"), (be(2), None), (be(3), b""), (be(4), b"four" * 300), (b"longer-key-than-8", b"x")]
    items.sort()
    base = str(tmp_path / "t")
    write_sstable(base, items, writer_options=(S.EnableBloomFilter(), S.BloomExpectedNumberOfElements(len(items))))
    qs = [k for k, _ in items] + [b"", be(0), be(5), b"longer-key-than-9", b"longer-k", be(2) + b"\0"] + [be(i) for i in range(100, 400)]
    for path, extra in ((base, ()), (_golden_with_filter(tmp_path, "sstables", "SimpleWriteHappyPathSSTableWithCRCHashesMismatch",
                                                         "SimpleWriteHappyPathSSTableWithCRCHashesMismatch"),
                                     (S.SkipHashCheckOnLoad(),))):
        r, err = S.NewSSTableReader(S.ReadBasePath(path), *opts, *extra)
        assert err is None, err
        assert r.bloomFilter is not None
        queries = qs + [be(i) for i in range(0, 9)]
        gets = [r.Get(q) for q in queries]
        _same(r.GetBatch(queries), gets)
        _same(r.ContainsBatch(queries), [r.Contains(q) for q in queries])
        _same(r.GetBatch(queries[:3]), gets[:3])  # the prefixes built once serve the next batch
        assert r.GetBatch([]) == [] and r.ContainsBatch([]) == []
        if path != base:  # entry be(4) fails its checksum: reported on reads only when they are checked
            bad = [q for q, (_, e) in zip(queries, gets) if e is not None and e is not S.NotFound]
            assert bad == ([q for q in queries if q == be(4)] if check_reads else [])
            assert all("Checksum mismatch" in str(e) for q, (_, e) in zip(queries, gets) if q in bad)
        else:  # the nil value and the empty value
            assert (gets[1], gets[2]) == ((None, None), (b"", None))
    # a table without a filter: ContainsBatch is the plain index lookup
    plain = open_table(str(tmp_path / "plain"), items, *opts)
    assert plain.bloomFilter is None
    _same(plain.ContainsBatch(qs), [plain.Contains(q) for q in qs])
    _same(plain.GetBatch(qs), [plain.Get(q) for q in qs])


GOLDEN_TABLES = [
    # (golden directory, table, filter fixture): the reference's WithBloom table is not among the golden v1 tables,
    # its filter goes with WithMetaData's table, which holds the same seven keys
    ("sstables", "SimpleWriteHappyPathSSTableWithMetaData", "SimpleWriteHappyPathSSTableWithBloom"),
    ("sstables", "SimpleWriteHappyPathSSTableWithMetaData", "SimpleWriteHappyPathSSTableWithMetaData"),
    ("sstables", "SimpleWriteHappyPathSSTableRecordIOV2", "SimpleWriteHappyPathSSTableRecordIOV2"),
    ("sstables", "SimpleWriteHappyPathSSTableWithCRCHashes", "SimpleWriteHappyPathSSTableWithCRCHashes"),
    ("sstables_v0_compat", "SimpleWriteHappyPathSSTableWithBloom", "v0_compat/SimpleWriteHappyPathSSTableWithBloom"),
    ("sstables_v0_compat", "SimpleWriteHappyPathSSTableWithMetaData", "v0_compat/SimpleWriteHappyPathSSTableWithMetaData"),
    ("sstables_v0_compat", "SimpleWriteHappyPathSSTableRecordIOV2", "v0_compat/SimpleWriteHappyPathSSTableRecordIOV2"),
]


@pytest.mark.parametrize("table_dir,table,fixture", GOLDEN_TABLES, ids=[g[2] for g in GOLDEN_TABLES])
def test_golden_table_with_its_reference_filter(tmp_path, table_dir, table, fixture):
    """TestSimpleHappyPathBloomRead and TestNegativeContainHappyPathBloom (sstable_reader_test.go:43,195)."""
    r, err = S.NewSSTableReader(S.ReadBasePath(_golden_with_filter(tmp_path, table_dir, table, fixture)))
    assert err is None, err
    assert r.bloomFilter is not None and r.bloomFilter.N() >= 7
    present = [be(i) for i in range(1, 8)]
    negative = [b"", b"\x01", b"\x01\x02\x03"]  # assertNegativeContains (:305-324)
    for k in present:
        assert r.Contains(k) == (True, None)
    for k in negative + [be(0), be(8), be(59)]:
        assert r.Contains(k) == (False, None)
        assert r.Get(k)[1] is S.NotFound
    qs = present + negative + [be(i) for i in range(0, 60)]
    assert r.ContainsBatch(qs) == [r.Contains(k) for k in qs]
    assert [f for f, _ in r.ContainsBatch(qs)] == [True] * 7 + [False] * 3 + [1 <= i <= 7 for i in range(60)]
    _same(r.GetBatch(qs), [r.Get(k) for k in qs])


def test_a_filter_that_does_not_read_fails_the_open(tmp_path):
    base = _golden_with_filter(tmp_path, "sstables", "SimpleWriteHappyPathSSTableWithMetaData",
                               "SimpleWriteHappyPathSSTableWithMetaData")
    path = os.path.join(base, "bloom.bf.gz")
    raw = open(path, "rb").read()
    os.remove(path)  # the copy keeps the fixture's mode, which may be read-only
    with open(path, "wb") as fh:
        fh.write(raw[:40])
    r, err = S.NewSSTableReader(S.ReadBasePath(base))
    assert r is None and f"error while reading bloom filterin '{path}': " in str(err)
    assert str(err).startswith(f"error while reading filter of sstable in '{base}': ")


def _check_written_filter(path, keys, want_mk):
    assert sorted(os.listdir(path)) == FILES4
    f = bm.parse(open(os.path.join(path, "bloom.bf.gz"), "rb").read())
    r, err = S.NewSSTableReader(S.ReadBasePath(path))
    assert err is None, err
    assert f.n == r.MetaData().numRecords == len(keys)
    assert (f.m, f.k) == want_mk
    assert all(f.contains(k) for k in keys)
    assert f.words == model_of(f.m, f.keys, keys).words  # apart from its random hash keys, the model's filter
    assert r.ContainsBatch(keys) == [(True, None)] * len(keys)
    return f


def test_merge_flush_and_recovery_write_the_filter(tmp_path):
    import wal as W
    from simpledb import proto as P

    bloom_opts = (S.EnableBloomFilter(), S.BloomExpectedNumberOfElements(500), S.BloomFalsePositiveProbability(0.02))
    want_mk = bm.optimal(500, 0.02)
    # a merge of three small tables
    tables = [[(be(k), b"t%d" % t) for k in range(t * 40, t * 40 + 100)] for t in range(3)]
    readers = []
    for t, items in enumerate(tables):
        readers.append(open_table(str(tmp_path / f"in{t}"), items))
    merged = sorted({k for items in tables for k, _ in items})
    with_f, without = str(tmp_path / "merge_f"), str(tmp_path / "merge")
    assert S.NewSSTableMerger().MergeCompact(readers, with_f, S.ScanReduceLatestWins, writer_options=bloom_opts) is None
    f1 = _check_written_filter(with_f, merged, want_mk)
    assert S.NewSSTableMerger().MergeCompact(readers, without, S.ScanReduceLatestWins) is None
    assert sorted(os.listdir(without)) == FILES3
    for name in FILES3:  # the filter changes nothing in the three other files
        assert open(os.path.join(with_f, name), "rb").read() == open(os.path.join(without, name), "rb").read()
    # Merge (every entry) over disjoint tables
    disjoint = [open_table(str(tmp_path / f"dis{t}"), [(be(1000 * t + i), b"v") for i in range(50)]) for t in range(3)]
    merge_all = str(tmp_path / "merge_all")
    assert S.NewSSTableMerger().Merge(disjoint, merge_all, writer_options=bloom_opts) is None
    f2 = _check_written_filter(merge_all, [be(1000 * t + i) for t in range(3) for i in range(50)], want_mk)
    assert f1.keys != f2.keys  # fresh random hash keys per filter
    # a flush
    ms = MS.NewMemStore()
    rng = random.Random(13)
    for i in range(600):
        key = b"user/%03d" % rng.randrange(200)
        if rng.random() < 0.8:
            assert ms.Upsert(key, rng.randbytes(10)) is None
        else:
            ms.Tombstone(key)
    live = sorted(k for k, v in ms._latest.items() if v is not None)
    every = sorted(ms._latest)
    assert len(live) < len(every)
    flushed, flushed_t, flushed_plain = str(tmp_path / "flush_f"), str(tmp_path / "flush_t"), str(tmp_path / "flush")
    assert ms.Flush(S.WriteBasePath(flushed), *bloom_opts) is None
    _check_written_filter(flushed, live, want_mk)
    assert ms.FlushWithTombstones(S.WriteBasePath(flushed_t), *bloom_opts) is None
    _check_written_filter(flushed_t, every, want_mk)
    assert ms.Flush(S.WriteBasePath(flushed_plain)) is None
    assert sorted(os.listdir(flushed_plain)) == FILES3
    # recover_wal: the filter is sized for the memstore's size
    for name, kw in (("rec_f", {"bloom_filter": True}), ("rec", {})):
        wal_dir, table = str(tmp_path / (name + "_wal")), str(tmp_path / name)
        os.makedirs(wal_dir)
        opts, err = W.NewWriteAheadLogOptions(W.BasePath(wal_dir), W.MaximumWalFileSizeBytes(4 << 10), W.WriterFactory(
            lambda p: __import__("recordio").NewFileWriter(p, L.COMP_SNAPPY)))
        assert err is None, err
        a, err = W.NewAppender(opts)
        assert err is None, err
        rng = random.Random(14)
        state = {}
        for i in range(400):
            key = b"wal/%03d" % rng.randrange(150)
            if rng.random() < 0.8:
                state[key] = True
                assert a.Append(P.marshal_upsert(key, rng.randbytes(20))) is None
            else:
                state[key] = False
                assert a.Append(P.marshal_delete(key)) is None
        assert a.Close() is None
        n, wrote, err = DB.recover_wal(wal_dir, table, **kw)
        assert err is None and (n, wrote) == (400, True)
        if kw:
            _check_written_filter(table, sorted(state), bm.optimal(len(state), 0.01))
        else:
            assert sorted(os.listdir(table)) == FILES3


def test_sst_bloom_add_argument_and_state_errors():
    lib = L.lib()
    h = ctypes.c_void_p()
    assert lib.rio_ctx_create(0, ctypes.byref(h)) == L.RIO_OK
    try:
        f = DevFilter(9586, hash_keys(7, 1))
        src = torch.zeros(4, dtype=torch.int64, device="cuda")
        assert lib.rio_sst_bloom_add(h, f.ref(), src.data_ptr(), 4, None) == L.RIO_ERR_STATE  # no plan on this context
        assert lib.rio_sst_bloom_add(h, f.ref(), src.data_ptr(), 0, None) == L.RIO_ERR_STATE
        torch.cuda.synchronize()
        assert not f.words().any()
    finally:
        lib.rio_ctx_destroy(h)
