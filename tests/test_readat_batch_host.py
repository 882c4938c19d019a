"""The batched ReadNextAt's test files and argument checks (CPU).

The oracle's read_next_at over each family of tests/readat_batch_cases.py reaches every status class the family is
named for, so the device test that compares every offset with the oracle (tests/test_gpu_readat_batch.py) meets them
all. The three new calls check their arguments before any device call, and librio exports them.
"""
import ctypes

import pytest

import oracle_py as orc
import readat_batch_cases as cases
from conftest import STATUS as S
from recordio import _lib as L


def _statuses(img, offsets):
    out = {}
    for off in offsets:
        st, rec = orc.read_next_at(img, off)
        key = "NIL" if st == 0 and rec is None else st
        out.setdefault(key, off)
    return out


@pytest.fixture(scope="module")
def sweep():
    return dict(cases.sweep_files())


def test_sweep_files_reach_their_status_classes(sweep):
    assert len(sweep) == 32 and all(len(img) <= 4096 for img in sweep.values())
    for name, img in sweep.items():
        codec, version, kind = name.split("_")
        seen = _statuses(img, range(len(img) + 3))
        want = {S["OK"], S["INVALID_OFFSET"], S["MAGIC"]}
        if version == "v1":  # v1 reads a fixed 20 bytes: that read runs short near the file's end, and at it too
            want |= {S["EOF_HEADER"]}
        else:
            want |= {S["EOF"]}
            if kind == "cut" and codec in ("none", "snappy"):  # the cut leaves a magic number and one more byte
                want |= {S["EOF_HEADER"]}
        if version in ("v3", "v4"):
            want |= {"NIL"}
        if version == "v4" and kind == "tail":
            want |= {S["HEADER_CRC"]}
        if kind == "cut":
            want |= {S["EOF_PAYLOAD"]}
        assert want <= set(seen), (name, sorted(map(str, want - set(seen))))
    # codec errors on a located payload: the bytes behind an offset inside a record, read as a header
    assert any(S["DECOMPRESS"] in _statuses(img, range(len(img))) for n, img in sweep.items() if n.startswith("snappy"))


def test_sweep_details_of_the_damaged_header(sweep):
    img = sweep["none_v4_tail"]
    hits = [orc.read_next_at(img, off, details=True) for off in range(len(img))]
    crc = [h for h in hits if h[0] == S["HEADER_CRC"]]
    assert crc and all(h[2] != h[3] for h in crc)


def test_snappy_families():
    img, recs = cases.snappy_forms()
    starts = cases.record_starts(img)
    assert len(starts) == len(recs)
    for off, want in zip(starts, recs):
        assert orc.read_next_at(img, off) == (0, want)
    assert recs[-1] == b"" and len(recs[3]) > cases.K_COOP_RING
    img, recs = cases.snappy_corrupt()
    starts = cases.record_starts(img)
    assert len(starts) == len(recs) == 9
    for off, want in zip(starts, recs):
        st, rec = orc.read_next_at(img, off)
        assert (st, rec) == ((0, want) if want is not None else (S["DECOMPRESS"], None)), off
    assert [r is None for r in recs] == [False, True] * 4 + [False]


def test_plain_lengths():
    img, recs = cases.plain_lengths()
    assert [len(r) for r in recs] == list(cases.PLAIN_LENGTHS)
    for off, want in zip(cases.record_starts(img), recs):
        assert orc.read_next_at(img, off) == (0, want)


def test_symbols_exported_and_bound():
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ("rio_device_read_at_plan", "rio_device_read_at_copy", "rio_reader_read_next_at_batch"):
        assert hasattr(lib, name) and name in L.EXPORTED
    assert ctypes.sizeof(L.ReadAtHit) == 48


def test_argument_errors_come_before_any_device_call():
    """No GPU here: a call that reached the device would return RIO_ERR_HIP (or crash on the null context)."""
    lib = L.lib()
    buf = (ctypes.c_uint64 * 16)()
    p = ctypes.addressof(buf)
    aligned = (p + 15) & ~15
    ctx = ctypes.c_void_p(p)  # never dereferenced: every call below fails on another argument first
    big = (1 << 31) - 1
    # plan
    assert lib.rio_device_read_at_plan(None, aligned, 8, p, 1, p, p, None) == L.RIO_ERR_ARG
    assert lib.rio_device_read_at_plan(ctx, None, 8, p, 1, p, p, None) == L.RIO_ERR_ARG
    assert lib.rio_device_read_at_plan(ctx, aligned + 1, 8, p, 1, p, p, None) == L.RIO_ERR_ARG
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.rio_device_read_at_plan(ctx, aligned, 8, args[0], 1, args[1], args[2], None) == L.RIO_ERR_ARG
    assert lib.rio_device_read_at_plan(ctx, aligned, 8, p, big, p, p, None) == L.RIO_ERR_UNSUPPORTED
    assert lib.rio_device_read_at_plan(ctx, aligned, 8, None, 0, None, None, None) == L.RIO_OK
    # copy
    assert lib.rio_device_read_at_copy(None, aligned, 8, 1, p, p, p, 64, None) == L.RIO_ERR_ARG
    assert lib.rio_device_read_at_copy(ctx, None, 8, 1, p, p, p, 64, None) == L.RIO_ERR_ARG
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.rio_device_read_at_copy(ctx, aligned, 8, 1, args[0], args[1], args[2], 64, None) == L.RIO_ERR_ARG
    assert lib.rio_device_read_at_copy(ctx, aligned, 8, big, p, p, p, 64, None) == L.RIO_ERR_UNSUPPORTED
    assert lib.rio_device_read_at_copy(ctx, aligned, 8, 0, None, None, None, 0, None) == L.RIO_OK
    # the handle
    data, off = ctypes.c_void_p(), ctypes.POINTER(ctypes.c_uint64)()
    hits = (L.ReadAtHit * 1)()
    f = lib.rio_reader_read_next_at_batch
    assert f(None, buf, 1, hits, ctypes.byref(data), ctypes.byref(off)) == L.RIO_ERR_ARG
    r = ctypes.c_void_p()  # a reader that was never opened holds its context without using it
    assert lib.rio_reader_new_mmap(ctx, __file__.encode(), ctypes.byref(r)) == L.RIO_OK
    try:
        assert f(r, None, 1, hits, ctypes.byref(data), ctypes.byref(off)) == L.RIO_ERR_ARG
        assert f(r, buf, 1, None, ctypes.byref(data), ctypes.byref(off)) == L.RIO_ERR_ARG
        assert f(r, buf, 1, hits, None, ctypes.byref(off)) == L.RIO_ERR_ARG
        assert f(r, buf, 1, hits, ctypes.byref(data), None) == L.RIO_ERR_ARG
        assert f(r, buf, big, hits, ctypes.byref(data), ctypes.byref(off)) == L.RIO_ERR_UNSUPPORTED
        assert f(r, buf, 1, hits, ctypes.byref(data), ctypes.byref(off)) == L.RIO_ERR_STATE
    finally:
        lib.rio_reader_free(r)
