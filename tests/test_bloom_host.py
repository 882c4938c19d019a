"""The tables' bloom filter on the host (no GPU): the model (tests/bloom_model.py) and sstables.bloom.Filter
against the reference's nine bloom.bf.gz fixtures (tests/golden/bloom), serialisation, refusals, the sizing
formula, the C-ABI's argument checks and the writer options."""
import ctypes
import glob
import gzip
import json
import os
import random
import struct

import pytest

import bloom_model as bm
from conftest import GOLDEN

import sstables
from recordio import _lib as L
from sstables import bloom

ROOT = os.path.join(GOLDEN, "bloom")
with open(os.path.join(ROOT, "fixtures.json")) as _f:
    FIXTURES = json.load(_f)
NAMES = sorted(FIXTURES)


def be32(i: int) -> bytes:
    return struct.pack(">I", i)


def raw(name: str) -> bytes:
    with open(os.path.join(ROOT, name, "bloom.bf.gz"), "rb") as f:
        return f.read()


def test_nine_fixtures_on_disk():
    found = sorted(os.path.relpath(os.path.dirname(p), ROOT)
                   for p in glob.glob(os.path.join(ROOT, "**", "bloom.bf.gz"), recursive=True))
    assert found == NAMES and len(NAMES) == 9
    # the issue's membership table: 1..7 in the eight 7-key files, 42 and 45 in ...EmptyValues
    for name, e in FIXTURES.items():
        assert e["members"] == ([42, 45] if name.endswith("EmptyValues") else list(range(1, 8))), name
    assert FIXTURES["v0_compat/SimpleWriteHappyPathSSTableWithBloom"]["n"] == 72
    assert (FIXTURES["SimpleWriteHappyPathSSTableWithBloom"]["m"], FIXTURES["SimpleWriteHappyPathSSTableWithBloom"]["k"]) == (9586, 7)
    assert (FIXTURES["v0_compat/SimpleWriteHappyPathSSTableWithBloom"]["m"],
            FIXTURES["v0_compat/SimpleWriteHappyPathSSTableWithBloom"]["k"]) == (4606, 4)


@pytest.mark.parametrize("name", NAMES)
def test_model_parses_fixture(name):
    e = FIXTURES[name]
    f = bm.parse(raw(name))  # checks the length and the SHA-384 trailer
    assert (f.k, f.n, f.m, f.popcount()) == (e["k"], e["n"], e["m"], e["popcount"])
    assert [i for i in range(60) if f.contains(be32(i))] == e["members"]
    assert gzip.decompress(raw(name)) == f.payload()


@pytest.mark.parametrize("name", NAMES)
def test_filter_parses_fixture(name):
    e = FIXTURES[name]
    f, err = bloom.ReadFile(os.path.join(ROOT, name, "bloom.bf.gz"))
    assert err is None
    assert (f.K(), f.N(), f.M()) == (e["k"], e["n"], e["m"])
    assert sum(bin(b).count("1") for b in f.bits) == e["popcount"]
    assert [i for i in range(60) if f.Contains(be32(i))] == e["members"]
    model = bm.parse(raw(name))
    assert f.payload() == model.payload() and list(f.keys) == list(model.keys)


def test_fnv1_not_fnv1a():
    assert bloom.fnv1_64(b"") == bm.fnv1_64(b"") == 0xCBF29CE484222325
    assert bloom.fnv1_64(b"a") == bm.fnv1_64(b"a") == 0xAF63BD4C8601B7BE  # FNV-1; FNV-1a gives af63dc4c8601ec8c
    rng = random.Random(3)
    for n in (1, 7, 8, 9, 33):
        k = bytes(rng.randrange(256) for _ in range(n))
        assert bloom.fnv1_64(k) == bm.fnv1_64(k)


def test_write_read_round_trip(tmp_path):
    f, err = bloom.NewOptimal(1000, 0.01)
    assert err is None and (f.M(), f.K()) == (9586, 7)
    keys = [be32(i) for i in range(0, 300, 3)] + [b"", b"a", b"a\0"]
    for k in keys:
        f.Add(k)
    path = str(tmp_path / "bloom.bf.gz")
    assert f.WriteFile(path) is None
    g, err = bloom.ReadFile(path)
    assert err is None
    assert (g.M(), g.K(), g.N(), g.keys, g.bits) == (f.M(), f.K(), len(keys), f.keys, f.bits)
    model = bm.parse(open(path, "rb").read())  # the model reads what the package wrote
    assert model.n == len(keys) and all(model.contains(k) for k in keys)
    rebuilt = bm.Model(f.m, f.keys)
    for k in keys:
        rebuilt.add(k)
    assert rebuilt.payload() == f.payload()
    # two filters never share their random hash keys
    h, _ = bloom.NewOptimal(1000, 0.01)
    assert h.keys != f.keys


def test_new_with_given_keys_and_limits():
    f, err = bloom.New(64, 3, keys=[1, 2, 3])
    assert err is None and (f.m, f.k, f.keys) == (64, 3, [1, 2, 3])
    for m, k in ((1, 3), (0, 1), (64, 0)):
        f, err = bloom.New(m, k)
        assert f is None and err is not None
    for n, p in ((0, 0.01), (10, 0.0), (10, 1.0), (10, -0.5), (10, float("nan"))):
        f, err = bloom.NewOptimal(n, p)
        assert f is None and err is not None


def test_refusals(tmp_path):
    good = raw("SimpleWriteHappyPathSSTableWithBloom")
    body = bytearray(gzip.decompress(good))
    cases = {}
    flipped = bytearray(body)
    flipped[30] ^= 0x10  # a hash key byte: the trailer no longer matches
    cases["flipped"] = gzip.compress(bytes(flipped))
    bits = bytearray(body)
    bits[24 + 8 * 7 + 5] ^= 0x01  # a bit word byte
    cases["flipped_bits"] = gzip.compress(bytes(bits))
    cases["short_payload"] = gzip.compress(bytes(body[:-8]))
    cases["trailing_bytes"] = gzip.compress(bytes(body) + b"\0" * 8)
    cases["truncated_file"] = good[:len(good) // 2]
    cases["empty_file"] = b""
    cases["not_gzip"] = bytes(body)
    for name, img in cases.items():
        f, err = bloom.parse(img)
        assert f is None and err is not None, name
        with pytest.raises(ValueError):
            bm.parse(img)
    # any valid gzip reads: another compression level, another header
    f, err = bloom.parse(gzip.compress(bytes(body), compresslevel=1))
    assert err is None and f.payload() == bytes(body)
    f, err = bloom.ReadFile(str(tmp_path / "missing.bf.gz"))
    assert f is None and err is not None


@pytest.mark.parametrize("max_n,p,want", [(1000, 0.01, (9586, 7)), (1, 0.5, None), (10 ** 7, 0.01, None),
                                          (7, 1e-9, (302, 30))])
def test_optimal_against_model(max_n, p, want):
    m, k = ctypes.c_uint64(), ctypes.c_uint64()
    assert L.lib().rio_bloom_optimal(max_n, p, ctypes.byref(m), ctypes.byref(k)) == L.RIO_OK
    assert (m.value, k.value) == bm.optimal(max_n, p)
    if want is not None:
        assert (m.value, k.value) == want
    assert bloom.optimal(max_n, p) == (m.value, k.value)


def test_optimal_argument_errors():
    lib = L.lib()
    m, k = ctypes.c_uint64(), ctypes.c_uint64()
    for max_n, p in ((0, 0.01), (5, 0.0), (5, 1.0), (5, 1.5), (5, -1.0), (5, float("nan"))):
        assert lib.rio_bloom_optimal(max_n, p, ctypes.byref(m), ctypes.byref(k)) == L.RIO_ERR_ARG, (max_n, p)
    assert lib.rio_bloom_optimal(5, 0.01, None, ctypes.byref(k)) == L.RIO_ERR_ARG
    assert lib.rio_bloom_optimal(5, 0.01, ctypes.byref(m), None) == L.RIO_ERR_ARG


def test_device_calls_refuse_arguments_before_any_device_call():
    """RIO_ERR_ARG comes back before the context or the device is touched: the calls are made with a placeholder
    context and placeholder device pointers on a machine that may have no GPU."""
    lib = L.lib()
    ctx, ptr = ctypes.c_void_p(8), ctypes.c_void_p(64)

    def view(m=9586, k=7, bits=64, keys=64):
        return L.BloomView(bits=bits, hash_keys=keys, m=m, k=k)

    ok = view()
    sst = L.SstView(index=64, key_off=64, key_len=64, data=64, data_off=64, flags=64, crc=64, n=5, index_bytes=10,
                    data_bytes=10)
    add = lambda c, f, keys=ptr, off=ptr, n=3: lib.rio_bloom_add(c, f, keys, off, n, 10, None)  # noqa: E731
    has = lambda c, f, keys=ptr, off=ptr, hit=ptr, n=3: lib.rio_bloom_contains(c, f, keys, off, n, 10, hit, None)  # noqa: E731
    for call in (add, has):
        assert call(None, ctypes.byref(ok)) == L.RIO_ERR_ARG
        assert call(ctx, None) == L.RIO_ERR_ARG
        for bad in (view(k=0), view(k=L.RIO_BLOOM_MAX_K + 1), view(m=0), view(m=1), view(bits=None), view(keys=None)):
            assert call(ctx, ctypes.byref(bad)) == L.RIO_ERR_ARG
        assert call(ctx, ctypes.byref(ok), keys=None) == L.RIO_ERR_ARG
        assert call(ctx, ctypes.byref(ok), off=None) == L.RIO_ERR_ARG
        assert call(ctx, ctypes.byref(ok), n=0) == L.RIO_OK  # a no-op: nothing is touched
        assert call(ctx, ctypes.byref(view(k=0)), n=0) == L.RIO_ERR_ARG
    assert has(ctx, ctypes.byref(ok), hit=None) == L.RIO_ERR_ARG
    # rio_sst_bloom_add: arguments first (the plan state needs a real context)
    assert lib.rio_sst_bloom_add(None, ctypes.byref(ok), ptr, 3, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_bloom_add(ctx, None, ptr, 3, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_bloom_add(ctx, ctypes.byref(view(k=65)), ptr, 3, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_bloom_add(ctx, ctypes.byref(view(m=1)), ptr, 3, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_bloom_add(ctx, ctypes.byref(ok), None, 3, None) == L.RIO_ERR_ARG
    # rio_sst_key_prefixes
    assert lib.rio_sst_key_prefixes(None, ctypes.byref(sst), ptr, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_key_prefixes(ctx, None, ptr, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_key_prefixes(ctx, ctypes.byref(sst), None, None) == L.RIO_ERR_ARG
    empty = L.SstView(n=0)
    assert lib.rio_sst_key_prefixes(ctx, ctypes.byref(empty), None, None) == L.RIO_OK
    # rio_sst_lookup
    look = lambda c, v, pfx=ptr, f=None, keys=ptr, off=ptr, n=3, out=ptr: lib.rio_sst_lookup(  # noqa: E731
        c, v, pfx, f, keys, off, n, 10, out, None)
    assert look(None, ctypes.byref(sst)) == L.RIO_ERR_ARG
    assert look(ctx, None) == L.RIO_ERR_ARG
    assert look(ctx, ctypes.byref(sst), pfx=None) == L.RIO_ERR_ARG
    assert look(ctx, ctypes.byref(sst), keys=None) == L.RIO_ERR_ARG
    assert look(ctx, ctypes.byref(sst), off=None) == L.RIO_ERR_ARG
    assert look(ctx, ctypes.byref(sst), out=None) == L.RIO_ERR_ARG
    assert look(ctx, ctypes.byref(sst), f=ctypes.byref(view(k=0))) == L.RIO_ERR_ARG
    assert look(ctx, ctypes.byref(sst), f=ctypes.byref(view(m=1))) == L.RIO_ERR_ARG
    assert look(ctx, ctypes.byref(sst), f=ctypes.byref(view(bits=None))) == L.RIO_ERR_ARG
    assert look(ctx, ctypes.byref(sst), n=0) == L.RIO_OK


def test_writer_options(tmp_path):
    o = sstables._WriterOpts()
    assert (o.enableBloomFilter, o.bloomExpectedNumberOfElements, o.bloomFpProbability) == (False, 1000, 0.01)
    assert sstables.writer_filter(o) == (None, None)  # off unless enabled
    sstables.EnableBloomFilter()(o)
    f, err = sstables.writer_filter(o)
    assert err is None and (f.M(), f.K(), f.N()) == (9586, 7, 0)
    sstables.BloomExpectedNumberOfElements(7)(o)
    sstables.BloomFalsePositiveProbability(1e-9)(o)
    f, err = sstables.writer_filter(o)
    assert err is None and (f.M(), f.K()) == (302, 30)
    sstables.BloomExpectedNumberOfElements(0)(o)
    f, err = sstables.writer_filter(o)
    assert f is None and str(err) == "unexpected number of bloom filter elements, was: 0"
    # the entry points return it before any device work
    opts = (sstables.WriteBasePath(str(tmp_path / "t")), sstables.EnableBloomFilter(), sstables.BloomExpectedNumberOfElements(0))
    from memstore import NewMemStore

    ms = NewMemStore()
    ms.Add(b"k", b"v")
    assert str(ms.Flush(*opts)) == "unexpected number of bloom filter elements, was: 0"
    assert str(ms.FlushWithTombstones(*opts)) == "unexpected number of bloom filter elements, was: 0"
    err = sstables.NewSSTableMerger().Merge([], str(tmp_path / "m"), writer_options=opts[1:])
    assert str(err) == "unexpected number of bloom filter elements, was: 0"
    w, err = sstables.NewSSTableStreamWriter(str(tmp_path / "w"), writer_options=opts[1:])
    assert w is None and str(err) == "unexpected number of bloom filter elements, was: 0"
    assert not os.path.exists(tmp_path / "t") and not os.path.exists(tmp_path / "m")
    # a probability NewOptimal refuses
    sstables.BloomExpectedNumberOfElements(10)(o)
    sstables.BloomFalsePositiveProbability(1.0)(o)
    f, err = sstables.writer_filter(o)
    assert f is None and "error while creating bloomfilter" in str(err)
    # more probes than the device takes: refused for the device paths only
    sstables.BloomFalsePositiveProbability(1e-30)(o)
    f, err = sstables.writer_filter(o)
    assert f is None and isinstance(err, sstables.UnsupportedError)
    f, err = sstables.writer_filter(o, device_limits=False)
    assert err is None and f.K() > L.RIO_BLOOM_MAX_K


def test_host_writer_writes_the_filter(tmp_path):
    items = [(be32(i), b"v%d" % i) for i in range(1, 40)]
    base = str(tmp_path / "with")
    sstables.write_sstable(base, items, writer_options=(sstables.EnableBloomFilter(), sstables.BloomExpectedNumberOfElements(39)))
    assert sorted(os.listdir(base)) == ["bloom.bf.gz", "data.rio", "index.rio", "meta.pb.bin"]
    f = bm.parse(open(os.path.join(base, "bloom.bf.gz"), "rb").read())
    assert (f.n, (f.m, f.k)) == (39, bm.optimal(39, 0.01))
    rebuilt = bm.Model(f.m, f.keys)
    for k, _ in items:
        rebuilt.add(k)
    assert rebuilt.words == f.words
    plain = str(tmp_path / "without")
    sstables.write_sstable(plain, items)
    assert sorted(os.listdir(plain)) == ["data.rio", "index.rio", "meta.pb.bin"]


def test_model_false_positive_share():
    """NewOptimal(100 000, 0.01) filled with 100 000 keys: the share of 100 000 seeded absent keys the model
    reports present is below 0.015. The design point is 0.01 and the binomial deviation at this sample 0.0003,
    so 0.015 is more than 15 deviations out; a model whose probes ignore the hash keys (all k probes on one
    bit: the share of set bits, about 0.1) fails it."""
    n = 100_000
    m, k = bm.optimal(n, 0.01)
    rng = random.Random(20240611)
    f = bm.Model(m, [rng.getrandbits(64) for _ in range(k)])
    for i in range(n):
        f.add(struct.pack(">Q", i))
    fp = sum(f.contains(struct.pack(">Q", (1 << 40) + i)) for i in range(n))
    share = fp / n
    print(f"false positives: {fp} of {n} = {share:.5f} (m = {m}, k = {k})")
    assert share < 0.015
    assert all(f.contains(struct.pack(">Q", i)) for i in range(0, n, 997))


def test_array_model_equals_the_scalar_model():
    """bloom_model.words_fixed_np and sparse_words (what the GPU tests use for large inputs) against Model."""
    import numpy as np

    rng = random.Random(5)
    rows = np.frombuffer(rng.randbytes(4 * 3000), dtype=np.uint8).reshape(3000, 4)
    for m, k in ((96, 7), (9586, 7), (64, 1), ((1 << 32) + 9, 3)):
        hk = [rng.getrandbits(64) for _ in range(k)]
        keys = [r.tobytes() for r in rows]
        sparse = bm.sparse_words(m, hk, keys)
        if m < 1 << 20:
            f = bm.Model(m, hk)
            for key in keys:
                f.add(key)
            assert bm.words_fixed_np(m, hk, rows).tolist() == f.words
            assert sparse == {i: w for i, w in enumerate(f.words) if w}
        else:
            probes = {(bm.fnv1_64(key) ^ h) % m for key in keys for h in hk}
            assert sum(bin(w).count("1") for w in sparse.values()) == len(probes)
            assert all((sparse[i >> 6] >> (i & 63)) & 1 for i in probes)
