"""Batched ReadNextAt on the device (GPU): rio_device_read_at_plan / _copy and rio_reader_read_next_at_batch.

Every answer is checked against the oracle's read_next_at (tests/oracle_py.py), offset by offset; the files are
tests/readat_batch_cases.py's (tests/test_readat_batch_host.py shows which status classes they reach). The output arena
is filled with 0xA5 before the copy, and every byte outside the ranges the plan gave out has to keep that value.
"""
import ctypes
import random
import threading

import numpy as np
import pytest
import torch

import corpus
import oracle_py as orc
import readat_batch_cases as cases
from conftest import STATUS as S
from recordio import NewMemoryMappedReaderWithPath, generate
from recordio import _lib as L
from recordio.device import to_device_file

pytestmark = pytest.mark.gpu

HIT = np.dtype([("status", "<i4"), ("nil", "<i4"), ("len", "<u8"), ("detail0", "<u8"), ("detail1", "<u8"),
                ("hdr_len", "<u8"), ("payload_off", "<u8")])
assert HIT.itemsize == ctypes.sizeof(L.ReadAtHit)
FILL, GUARD = 0xA5, 64


def run_pair(img, offsets, cap_of=None):
    """plan + copy over `offsets` of the file image -> (hits, out_off, out with its guard bytes, out_cap).
    out_cap = cap_of(out_off[n]) (default: out_off[n] + GUARD); the arena is out_off[n] + GUARD bytes."""
    lib, ctx = L.lib(), L.default_ctx(0)
    d_file, flen = to_device_file(img)
    n = len(offsets)
    d_offs = torch.from_numpy(np.asarray(offsets, dtype=np.uint64).view(np.int64).copy()).cuda()
    d_hits = torch.full((max(n, 1) * HIT.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")
    d_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert lib.rio_device_read_at_plan(ctx, d_file.data_ptr(), flen, d_offs.data_ptr(), n, d_hits.data_ptr(),
                                       d_off.data_ptr(), None) == 0
    torch.cuda.synchronize()
    out_off = d_off.cpu().numpy().astype(np.uint64)
    need = int(out_off[n])
    cap = need + GUARD if cap_of is None else cap_of(need)
    d_out = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert lib.rio_device_read_at_copy(ctx, d_file.data_ptr(), flen, n, d_hits.data_ptr(), d_off.data_ptr(),
                                       d_out.data_ptr(), cap, None) == 0
    torch.cuda.synchronize()
    hits = d_hits.cpu().numpy()[:n * HIT.itemsize].view(HIT)
    assert np.array_equal(d_off.cpu().numpy().astype(np.uint64), out_off)  # the copy leaves the offsets alone
    return hits, out_off, d_out.cpu().numpy(), cap


def check_exact(img, offsets, res, what=""):
    """none / snappy files: every hit and every record equal the oracle's; nothing written outside the ranges."""
    hits, out_off, out, _ = res
    pos = 0
    for i, off in enumerate(offsets):
        st, rec, d0, d1 = orc.read_next_at(img, int(off), details=True)
        h = hits[i]
        ctx = (what, i, int(off), st, h)
        assert h["status"] == st, ctx
        assert h["nil"] == (1 if st == 0 and rec is None else 0), ctx
        assert h["len"] == (len(rec) if rec is not None else 0), ctx
        assert (h["detail0"], h["detail1"]) == ((d0, d1) if st == S["HEADER_CRC"] else (0, 0)), ctx
        assert out_off[i] == pos, ctx
        lo, hi = int(out_off[i]), int(out_off[i + 1])
        if st == S["DECOMPRESS"]:  # found by the decoder: the range stays, its bytes are unspecified
            assert hi >= lo, ctx
            out[lo:hi] = FILL
        else:
            assert hi - lo == (len(rec) if rec is not None else 0), ctx
            if rec:
                assert out[lo:hi].tobytes() == rec, ctx
                out[lo:hi] = FILL
        pos = hi
    assert int(out_off[len(offsets)]) == pos and len(out) == pos + GUARD, what
    assert (out == FILL).all(), what  # the guard, and (all ranges painted over) nothing else either


# ---- 1. every offset of every sweep file ----------------------------------------------------------
SWEEP = dict(cases.sweep_files())


@pytest.mark.parametrize("name", sorted(SWEEP))
def test_every_offset_of_a_sweep_file(name):
    img = SWEEP[name]
    offsets = list(range(len(img) + 3))
    res = run_pair(img, offsets)
    codec = name.split("_")[0]
    if codec in ("none", "snappy"):
        check_exact(img, offsets, res, name)
        return
    hits, out_off, out, _ = res
    assert not out_off.any() and (out == FILL).all(), name  # nothing is expanded on the device
    empty_payload = S["EOF_CODEC"] if codec == "gzip" else S["DECOMPRESS"]
    starts = orc.file_reader_decode(img)["rec_off"]
    next_start = dict(zip(starts, starts[1:]))
    seen_unsupported = 0
    for off in offsets:
        st, rec, d0, d1 = orc.read_next_at(img, off, details=True)
        h = hits[off]
        ctx = (name, off, st, h)
        located = (st == 0 and rec is not None) or st in (S["DECOMPRESS"], S["EOF_CODEC"])
        if located and h["status"] == S["UNSUPPORTED"]:
            seen_unsupported += 1
            assert h["nil"] == 0 and h["len"] > 0 and h["payload_off"] + h["len"] <= len(img), ctx
            assert h["payload_off"] == off + h["hdr_len"], ctx
            if off in next_start:
                assert h["payload_off"] + h["len"] == next_start[off], ctx
            continue
        assert h["status"] == st, ctx
        assert h["nil"] == (1 if st == 0 and rec is None else 0) and h["len"] == 0, ctx
        if located:  # the one codec failure the device answers itself: an empty payload
            assert st == empty_payload, ctx
        assert (h["detail0"], h["detail1"]) == ((d0, d1) if st == S["HEADER_CRC"] else (0, 0)), ctx
    assert seen_unsupported >= 4, name


# ---- 2. Snappy forms and corrupt streams ----------------------------------------------------------
@pytest.mark.parametrize("family", ["forms", "corrupt"])
def test_snappy_forms_and_corrupt_streams(family):
    img, recs = cases.snappy_forms() if family == "forms" else cases.snappy_corrupt()
    starts = cases.record_starts(img)
    offsets = starts + starts[::-1] + [starts[0] + 1, len(img)]  # each record twice, and two that are none
    res = run_pair(img, offsets)
    hits = res[0]
    want = [0 if r is not None else S["DECOMPRESS"] for r in recs]
    assert list(hits["status"][:len(starts)]) == want
    check_exact(img, offsets, res, family)


def test_plain_lengths_both_copy_kernels():
    img, recs = cases.plain_lengths()
    starts = cases.record_starts(img)
    offsets = starts[::-1] + starts
    res = run_pair(img, offsets)
    assert list(res[0]["len"]) == [len(r) for r in recs[::-1] + recs]
    check_exact(img, offsets, res, "plain")


# ---- 3. launch shapes -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_records():
    """Per codec: (image, record starts, decoded arena, its offsets) of 20 000 records of about 24 bytes."""
    out = {}
    for comp in (cases.NONE, cases.SNAPPY):
        img = bytes(generate(20_000, 24, comp, kind=1, seed=77))
        o = orc.file_reader_decode_arrays(img)
        assert o["n_records"] == 20_000 and not o["n_bad"]
        out[comp] = (img, o["rec_off"].astype(np.uint64), o["out"], o["out_off"].astype(np.int64))
    return out


def _records_of(arena, aoff, pick):
    """The records `pick` of a decoded arena back to back (what the batch's out holds), without a Python loop."""
    lens = (aoff[pick + 1] - aoff[pick]).astype(np.int64)
    begin = np.concatenate([[0], np.cumsum(lens)])[:-1]
    idx = np.repeat(aoff[pick] - begin, lens) + np.arange(int(lens.sum()), dtype=np.int64)
    return arena[idx], lens.astype(np.uint64)


WRAP_ALL = 1_100_000


@pytest.mark.parametrize("comp", [cases.NONE, cases.SNAPPY])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 20_000, WRAP_ALL])
def test_launch_shapes(small_records, comp, n):
    """n = 20 000: more queries than the 8 192 waves of the largest Snappy grid (k_readat_snappy's loop goes round
    again; the locate and copy grids still cover it in one pass). n = 1 100 000: more than k_readat_locate's 2 048 x 256
    lanes, than the 4 096 x 16 (and x 4) groups of the copy grids and than the 4 096 x 256 lanes of the capacity loop,
    so every stride loop of every kernel goes round again. Drawn with replacement: shuffled, with duplicates."""
    img, starts, arena, aoff = small_records[comp]
    rng = np.random.default_rng(n)
    pick = rng.integers(0, len(starts), size=n)
    if n > 1:
        pick[-1] = pick[0]
    hits, out_off, out, _ = run_pair(img, starts[pick])
    want, lens = _records_of(arena, aoff, pick)
    assert not hits["status"].any() and not hits["nil"].any()
    assert np.array_equal(hits["len"], lens)
    assert np.array_equal(out_off, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))
    assert np.array_equal(out[:len(want)], want)
    assert len(out) == len(want) + GUARD and (out[len(want):] == FILL).all()


# ---- 4. capacity ----------------------------------------------------------------------------------
@pytest.mark.parametrize("comp", [cases.NONE, cases.SNAPPY])
@pytest.mark.parametrize("n", [3000, WRAP_ALL])
def test_capacity_at_half_the_need(small_records, comp, n):
    """n = 1 100 000: the capacity rule's own loop (4 096 x 256 lanes) goes round again, marking as it goes."""
    img, starts, arena, aoff = small_records[comp]
    pick = np.random.default_rng(5).integers(0, len(starts), size=n)
    hits, out_off, out, cap = run_pair(img, starts[pick], cap_of=lambda need: need // 2)
    lens = (aoff[pick + 1] - aoff[pick]).astype(np.uint64)
    assert np.array_equal(out_off, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))  # the full need
    assert cap == int(out_off[-1]) // 2 and 0 < cap < int(out_off[-1])
    inside = out_off[1:] <= cap
    assert inside.any() and not inside.all()
    assert np.array_equal(hits["status"], np.where(inside, 0, S["CAPACITY"]))
    assert np.array_equal(hits["len"], lens) and not hits["nil"].any()  # the length is reported either way
    k = int(inside.sum())  # the ranges are ascending: the first k lie inside
    want, _ = _records_of(arena, aoff, pick[:k])
    assert np.array_equal(out[:len(want)], want)
    assert (out[len(want):] == FILL).all()  # nothing at or past out_cap, nor in the gap below it


# ---- 5. refused file header -----------------------------------------------------------------------
@pytest.mark.parametrize("name,status", [("v0", "VERSION"), ("comp300", "COMPRESSION_TYPE"), ("short", "SHORT_FILE_HEADER")])
def test_refused_file_header(name, status):
    good = bytes(corpus.encode_file([b"abc", b"defg"], 0))
    img = {"v0": corpus.file_header(0, 0) + good[8:], "comp300": corpus.file_header(4, 300) + good[8:],
           "short": good[:5]}[name]
    offsets = [0, 8, 9, len(img), len(img) + 5, 8]
    hits, out_off, out, _ = run_pair(img, offsets)
    assert list(hits["status"]) == [S[status]] * len(offsets)
    assert not hits["nil"].any() and not hits["len"].any() and not out_off.any()
    assert (out == FILL).all()


# ---- 6. the handle --------------------------------------------------------------------------------
def _open(tmp_path, img, name="f.rio"):
    p = tmp_path / name
    p.write_bytes(bytes(img))
    r, err = NewMemoryMappedReaderWithPath(str(p))
    assert err is None and r.Open() is None
    return r


def _batch(r, offsets):
    """rio_reader_read_next_at_batch -> [(status, record or None, detail0, detail1)]"""
    n = len(offsets)
    arr = (ctypes.c_uint64 * max(n, 1))(*offsets)
    hits = (L.ReadAtHit * max(n, 1))()
    data, off = ctypes.c_void_p(), ctypes.POINTER(ctypes.c_uint64)()
    rc = L.lib().rio_reader_read_next_at_batch(r._h, arr, n, hits, ctypes.byref(data), ctypes.byref(off))
    assert rc == 0, rc
    out = []
    for i in range(n):
        h = hits[i]
        rec = None
        if h.status == 0 and not h.nil:
            assert off[i + 1] - off[i] == h.len
            rec = ctypes.string_at(data.value + off[i], h.len) if h.len else b""
        else:
            assert off[i + 1] == off[i] and h.len == 0
        out.append((h.status, rec, h.detail0, h.detail1))
    return out


def _mixed_offsets(img, seed, n=120):
    """record starts, offsets inside records and offsets past the end, shuffled, with duplicates"""
    rng = random.Random(seed)
    starts = orc.file_reader_decode(img)["rec_off"]
    offs = [rng.choice(starts) for _ in range(n // 2)] + [rng.randrange(len(img)) for _ in range(n // 3)]
    offs += [len(img), len(img) + 1, len(img) + 1000, 0, 8, 8]
    rng.shuffle(offs)
    return offs


def _oracle(img, offsets):
    out = []
    for off in offsets:
        st, rec, d0, d1 = orc.read_next_at(img, off, details=True)
        out.append((st, rec) + ((d0, d1) if st == S["HEADER_CRC"] else (0, 0)))
    return out


@pytest.mark.parametrize("codec", sorted(cases.CODECS))
def test_handle_fresh_then_with_the_index_built(tmp_path, codec):
    """A fresh reader answers the batch without building its index (gzip / lzw records through readat_expand);
    after one ReadNextAt has built it, the same batch gives the same answers from the index and the device."""
    img = SWEEP[f"{codec}_v4_tail"]
    offsets = _mixed_offsets(img, 3)
    want = _oracle(img, offsets)
    r = _open(tmp_path, img)
    assert _batch(r, offsets) == want
    assert _batch(r, []) == []
    r.ReadNextAt(8)  # builds the index
    n_rec, _, _ = r.index_info()
    assert n_rec > 0
    assert _batch(r, offsets) == want
    r.Close()


def test_handle_takes_the_device_until_an_index_exists(tmp_path):
    """The batch builds no index (rio_reader_index_info would build one, so the check is on the path taken): the
    device's hits carry hdr_len / payload_off, the index's do not."""
    img, recs = cases.plain_lengths()
    starts = cases.record_starts(img)
    r = _open(tmp_path, img)
    n = len(starts)
    arr = (ctypes.c_uint64 * n)(*starts)
    hits = (L.ReadAtHit * n)()
    data, off = ctypes.c_void_p(), ctypes.POINTER(ctypes.c_uint64)()
    f = L.lib().rio_reader_read_next_at_batch
    assert f(r._h, arr, n, hits, ctypes.byref(data), ctypes.byref(off)) == 0
    assert all(h.hdr_len > 0 and h.payload_off == s + h.hdr_len for h, s in zip(hits, starts))  # the device's hits
    r.ReadNextAt(8)
    assert f(r._h, arr, n, hits, ctypes.byref(data), ctypes.byref(off)) == 0
    assert all(h.hdr_len == 0 for h in hits)  # now the index's
    assert [ctypes.string_at(data.value + off[i], off[i + 1] - off[i]) for i in range(n)] == recs
    r.Close()


def test_four_threads_batch_on_one_reader(tmp_path):
    img, _ = cases.snappy_forms()
    plans = [_mixed_offsets(img, 10 + t, n=60) for t in range(4)]
    wants = [_oracle(img, p) for p in plans]
    r = _open(tmp_path, img)
    go, bad = threading.Barrier(4), []

    def run(t):
        go.wait()
        for _ in range(3):
            if _batch(r, plans[t]) != wants[t]:
                bad.append(t)

    th = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not bad
    r.Close()


CORPUS = {n: img for n, img in corpus.cases()}


@pytest.mark.parametrize("name", ["mixed_c0_trunc2", "mixed_c2_trunc4", "damaged_small_c0", "damaged_small_c2", "v1_torn_header_12"])
def test_python_batch_equals_a_loop_of_read_next_at(tmp_path, name):
    img = bytes(CORPUS[name])
    offsets = _mixed_offsets(img, 9, n=90)
    r = _open(tmp_path, img)
    got = r.ReadNextAtBatch(offsets)  # before any single call: the device answers everything
    loop = [r.ReadNextAt(o) for o in offsets]
    again = r.ReadNextAtBatch(offsets)  # the index is built now
    for g, a, (rec, err), o in zip(got, again, loop, offsets):
        assert g[0] == rec and a[0] == rec, o
        assert str(g[1]) == str(err) and str(a[1]) == str(err), o
        assert (g[1] is None) == (err is None)
    r.Close()
