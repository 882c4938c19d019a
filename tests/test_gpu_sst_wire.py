"""The SSTable protobuf parsers on the device (GPU) against the plain model of tests/sst_wire_cases.py, at the
four places they run: k_sst_index (RawBytes), k_sst_data_entry (RawBytes with a base offset), k_index_search
(WinBytes: a 16-byte window per lane, at every file offset mod 16) and k_index_search_view (the pointer form over
a decoded arena); then one table whose every index record is a non-canonical encoding, end to end.

Hostile here means hostile bytes inside well-formed arenas: every offset array ascends and ends at the arena's
length, every arena has RIO_DEVICE_PAD bytes of slack. All comparisons are exact."""
import os
import re
import struct

import numpy as np
import pytest

import oracle_py as orc
import sst_wire_cases as W
from conftest import PKG
from recordio import _lib as L

pytestmark = pytest.mark.gpu

NONE = (1 << 64) - 1
_SRC = open(os.path.join(PKG, "csrc", "rio_sstable.hip")).read()
# launch_sst_index / launch_sst_data_entry: dim3((unsigned)(blocks < CAP ? blocks : CAP)), dim3(LANES)
_CAPS = set(re.findall(r"blocks < (\d+) \? blocks : (\d+)\)\), dim3\((\d+)\)", _SRC))
assert len(_CAPS) == 1, _CAPS
GRID_CAP, _cap2, LANES = (int(x) for x in next(iter(_CAPS)))
assert GRID_CAP == _cap2
ROUND = GRID_CAP * LANES
BIG_N = ROUND + 257

FAMILY = W.all_index_cases()
SEEDED = W.seeded_records(4000, 4000)
INDEX_RECORDS = [r for _, r in FAMILY] + SEEDED
INDEX_MODEL = [W.index_entry_model(r) for r in INDEX_RECORDS]
DATA_RECORDS = [r for _, r in W.data_family()] + [r for _, r in FAMILY] + SEEDED
DATA_MODEL = [W.data_entry_model(r) for r in DATA_RECORDS]
BAD_A = dict(W.index_families()["lengths"])["key of 2^32+3 with 3 bytes there"]
BAD_B = dict(W.index_families()["tags"])["field 2^32+1 bytes"]


def be(i):
    return struct.pack(">I", i)


def u64(t):
    """A device int64 tensor as unsigned 64-bit numpy."""
    return t.cpu().numpy().view(np.uint64)


def offsets(lens):
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    return off


def to_device(arena, off):
    """A host byte array and its ascending offsets -> (padded device arena, device offsets)."""
    import torch

    assert int(off[-1]) == len(arena) and np.all(np.diff(off.astype(np.int64)) >= 0)
    d = torch.zeros(len(arena) + L.RIO_DEVICE_PAD, dtype=torch.uint8, device="cuda:0")
    d[:len(arena)] = torch.from_numpy(np.array(arena, dtype=np.uint8))  # (a writable copy)
    return d, torch.from_numpy(off.view(np.int64).copy()).cuda()


def arena_of(records):
    arena = np.frombuffer(b"".join(records), dtype=np.uint8)
    return arena, offsets([len(r) for r in records])


def index_parse(arena, off):
    """rio_sst_index_parse -> (key_off, key_len, value_off, checksum, result[0]); the outputs start out as 0xA5."""
    import torch

    n = len(off) - 1
    d, doff = to_device(arena, off)
    outs = [torch.full((max(n, 1),), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda:0") for _ in range(4)]
    res = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    rc = L.lib().rio_sst_index_parse(L.default_ctx(0), d.data_ptr(), doff.data_ptr(), n, *(o.data_ptr() for o in outs),
                                     res.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return tuple(u64(o)[:n] for o in outs) + (int(u64(res)[0]),)


def data_entries(arena, off):
    """rio_sst_data_entries -> (view as [n, 2], result[0])"""
    import torch

    n = len(off) - 1
    d, doff = to_device(arena, off)
    view = torch.full((2 * max(n, 1),), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda:0")
    res = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    rc = L.lib().rio_sst_data_entries(L.default_ctx(0), d.data_ptr(), doff.data_ptr(), n, view.data_ptr(), res.data_ptr(),
                                      None)
    assert rc == 0
    torch.cuda.synchronize()
    return u64(view)[:2 * n].reshape(n, 2), int(u64(res)[0])


def first_rejected(model, bad=None):
    return next((i for i, m in enumerate(model) if m is bad), NONE)


def check_index(records, model):
    arena, off = arena_of(records)
    ko, kl, vo, cs, first = index_parse(arena, off)
    blob = arena.tobytes()
    for i, m in enumerate(model):
        if m is None:
            continue
        a, b = int(ko[i]), int(ko[i]) + int(kl[i])
        assert int(off[i]) <= a <= b <= int(off[i + 1]), (i, records[i].hex(), a, b)
        assert (blob[a:b], int(vo[i]), int(cs[i])) == m, (i, records[i].hex(), m)
    assert first == first_rejected(model), (first, first_rejected(model))


def test_index_parse_every_case_and_seeded():
    assert any(m is None for m in INDEX_MODEL)
    check_index(INDEX_RECORDS, INDEX_MODEL)
    valid = [(r, m) for r, m in zip(INDEX_RECORDS, INDEX_MODEL) if m is not None]
    assert len(valid) > 2000
    check_index([r for r, _ in valid], [m for _, m in valid])  # nothing malformed: ~0


def check_data(records, model):
    arena, off = arena_of(records)
    view, first = data_entries(arena, off)
    blob = arena.tobytes()
    for j, m in enumerate(model):
        b, e = int(view[j, 0]), int(view[j, 1])
        if m is W.BAD:
            assert (b, e) == (L.RIO_VALUE_BAD, L.RIO_VALUE_BAD), (j, records[j].hex())
        elif m is None:
            assert (b, e) == (L.RIO_VALUE_NIL, L.RIO_VALUE_NIL), (j, records[j].hex())
        else:
            assert int(off[j]) <= b <= e <= int(off[j + 1]) and blob[b:e] == m, (j, records[j].hex(), b, e, m)
    assert first == first_rejected(model, W.BAD)


def test_data_entries_every_case_and_seeded():
    assert any(m is W.BAD for m in DATA_MODEL) and any(m is None for m in DATA_MODEL)
    check_data(DATA_RECORDS, DATA_MODEL)
    valid = [(r, m) for r, m in zip(DATA_RECORDS, DATA_MODEL) if m is not W.BAD]
    check_data([r for r, _ in valid], [m for _, m in valid])


@pytest.mark.parametrize("low,high", [(BAD_A, BAD_B), (BAD_B, BAD_A)])
@pytest.mark.parametrize("which", ["index", "data"])
def test_two_malformed_records_in_different_blocks(which, low, high):
    """Indices 3 and 700 (blocks 0 and 2), each malformed record once at the smaller and once at the larger
    index: the smaller index is reported, whichever block finishes first."""
    records = [W.decorated(be(i), i, i, i) for i in range(900)]
    records[3], records[700] = low, high
    assert 3 // LANES != 700 // LANES
    arena, off = arena_of(records)
    first = index_parse(arena, off)[4] if which == "index" else data_entries(arena, off)[1]
    assert first == 3


# ---- one round of the grid and more ------------------------------------------------------------------------
def short_valid(records, model, bad):
    """The distinct accepted records under 16 bytes, in a tile whose length is no multiple of 64."""
    seen, out = set(), []
    for r, m in zip(records, model):
        if m is not bad and len(r) < 16 and r not in seen:
            seen.add(r)
            out.append((r, m))
    if len(out) % 64 == 0:
        out.pop()
    assert len(out) > 64 and len(out) % 64
    return out


def tiled_arena(tile, n, at, bad):
    """n records repeating `tile`, record `at` replaced by `bad` -> (arena, off, index into tile per record)."""
    reps = -(-n // len(tile))
    which = np.tile(np.arange(len(tile)), reps)[:n]
    lens = np.array([len(r) for r in tile], dtype=np.uint64)[which]
    lens[at] = len(bad)
    off = offsets(lens)
    whole = np.tile(np.frombuffer(b"".join(tile), dtype=np.uint8), reps)
    plain = offsets(np.array([len(r) for r in tile], dtype=np.uint64)[which])
    arena = np.concatenate([whole[:int(plain[at])], np.frombuffer(bad, dtype=np.uint8),
                            whole[int(plain[at + 1]):int(plain[n])]])
    return arena, off, which


def gathered(arena, begin, lens, width):
    """[n, width] bytes of arena[begin[i] : begin[i] + lens[i]), zero beyond each length."""
    cols = np.arange(width, dtype=np.int64)[None, :]
    mask = cols < lens.astype(np.int64)[:, None]
    idx = np.where(mask, begin.astype(np.int64)[:, None] + cols, 0)
    return np.where(mask, arena[idx], 0).astype(np.uint8)


def padded(values, width):
    out = np.zeros((len(values), width), dtype=np.uint8)
    for i, v in enumerate(values):
        out[i, :len(v)] = np.frombuffer(v, dtype=np.uint8)
    return out


def test_index_parse_beyond_one_round_of_the_grid():
    tile = short_valid(INDEX_RECORDS, INDEX_MODEL, None)
    at = ROUND + 100
    arena, off, which = tiled_arena([r for r, _ in tile], BIG_N, at, BAD_A)
    assert len(arena) < 12 << 20
    ko, kl, vo, cs, first = index_parse(arena, off)
    assert first == at
    keep = np.arange(BIG_N) != at
    want_kl = np.array([len(m[0]) for _, m in tile], dtype=np.uint64)[which]
    np.testing.assert_array_equal(kl[keep], want_kl[keep])
    np.testing.assert_array_equal(vo[keep], np.array([m[1] for _, m in tile], dtype=np.uint64)[which][keep])
    np.testing.assert_array_equal(cs[keep], np.array([m[2] for _, m in tile], dtype=np.uint64)[which][keep])
    assert np.all((ko >= off[:-1])[keep]) and np.all((ko + kl <= off[1:])[keep])
    ko, kl = np.where(keep, ko, 0), np.where(keep, kl, 0)
    want = padded([m[0] for _, m in tile], 16)[which]
    want[at] = 0
    np.testing.assert_array_equal(gathered(arena, ko, kl, 16), want)


def test_data_entries_beyond_one_round_of_the_grid():
    tile = short_valid(DATA_RECORDS, DATA_MODEL, W.BAD)
    assert any(m is None for _, m in tile) and any(m == b"" for _, m in tile)
    at = ROUND + 200
    arena, off, which = tiled_arena([r for r, _ in tile], BIG_N, at, BAD_B)
    assert len(arena) < 12 << 20
    view, first = data_entries(arena, off)
    assert first == at and view[at].tolist() == [L.RIO_VALUE_BAD] * 2
    nil = np.array([m is None for _, m in tile])[which]
    nil[at] = False
    assert np.all(view[nil] == np.uint64(L.RIO_VALUE_NIL))
    there = ~nil
    there[at] = False
    b, e = view[:, 0], view[:, 1]
    assert np.all(b[there] >= off[:-1][there]) and np.all(b[there] <= e[there]) and np.all(e[there] <= off[1:][there])
    want_len = np.array([len(m or b"") for _, m in tile], dtype=np.uint64)[which]
    np.testing.assert_array_equal((e - b)[there], want_len[there])
    want = padded([m or b"" for _, m in tile], 16)[which]
    want[~there] = 0
    np.testing.assert_array_equal(gathered(arena, np.where(there, b, 0), np.where(there, e - b, 0), 16), want)


# ---- k_index_search (WinBytes) and k_index_search_view -------------------------------------------------------
ACCEPTED = [(n, r) for (n, r), m in zip(FAMILY, INDEX_MODEL) if m is not None]
REJECTED = {n: r for (n, r), m in zip(FAMILY, INDEX_MODEL) if m is None}
PLANTED = {10: REJECTED["lengths: key of 2^32+3 with 3 bytes there"], 40: REJECTED["tags: field 2^32+1 bytes"],
           70: REJECTED["groups: 17 nested groups"]}


def search_key(j):
    return b"k%04d" % j + (b"", b"-" * 15, b"=" * 36)[j % 3]


def search_entries(r, planted=None):
    """-> (entries, keys): a canonical first entry whose key is r bytes longer than the shortest, then every accepted
    family case followed by a non-canonical encoding of an ascending key (the last occurrence of every field wins);
    `planted` replaces some entries by rejected records."""
    keys = [b"\x00ffff" + b"f" * r] + [search_key(j) for j in range(1, len(ACCEPTED) + 1)]
    entries = [W.field(1, keys[0])]
    for j, (_, case) in enumerate(ACCEPTED, 1):
        e = case + W.decorated(keys[j], 8 + 17 * j, j * 0x9E3779B97F4A7C15 & NONE, j)
        assert W.index_entry_model(e) == (keys[j], 8 + 17 * j, j * 0x9E3779B97F4A7C15 & NONE)
        entries.append((planted or {}).get(j, e))
    assert keys == sorted(keys)
    return entries, keys


def search_queries(keys):
    qs = list(keys) + [b"", b"\xff" * 40]
    for j, k in enumerate(keys):
        qs.append(k[:1 + (7 * j) % len(k)])
        if j % 2:
            qs.append(k[:-1] + b"~")
    assert len(qs) < 350
    return qs


def test_index_search_parses_every_entry_at_every_window_offset():
    """The first entry's key grows byte by byte until the records behind it have begun at every offset mod 16 (its
    v4 header holds varints of its own, so the shift is read from the record offsets, not taken as r)."""
    import test_gpu_disk_index as DI

    starts = {}
    for r in range(64):
        entries, keys = search_entries(r)
        img = DI.index_image(entries)
        rec_off = orc.file_reader_decode(bytes(img))["rec_off"]
        if rec_off[1] % 16 in starts:
            continue
        starts[rec_off[1] % 16] = rec_off
        got = DI.check(img, search_queries(keys))
        assert all(g[0] == 0 and g[2] for g in got[:len(keys)]), r  # every key found: every entry parsed
        assert [g[3] for g in got[1:len(keys)]] == [8 + 17 * j for j in range(1, len(keys))]
        if len(starts) == 16:
            break
    starts = np.array(list(starts.values()))
    assert starts.shape == (16, len(ACCEPTED) + 1)
    for j in range(1, starts.shape[1]):  # every decorated entry began at every offset mod 16
        assert sorted(starts[:, j] % 16) == list(range(16)), j
    lens = [len(e) for e in search_entries(0)[0]]
    assert sum(1 for n in lens if n > 32) > 20 and sum(1 for n in lens if 16 < n <= 32) >= 3


@pytest.mark.parametrize("r", [0, 5, 11])
def test_index_search_reports_planted_malformed_entries(r):
    import test_gpu_disk_index as DI

    entries, keys = search_entries(r, PLANTED)
    got = DI.check(DI.index_image(entries), search_queries(keys))  # RIO_ERR_PROTO exactly where the oracle says
    proto_errors = sum(1 for g in got if g[0] == L.RIO_ERR_PROTO)
    assert 3 <= proto_errors < len(got)


@pytest.mark.parametrize("comp", [1, 2, 3])
def test_index_search_view_on_decorated_entries(comp):
    import test_gpu_disk_index as DI

    for r, planted in ((0, None), (7, None), (3, PLANTED)):
        entries, keys = search_entries(r, planted)
        idx = DI.index_image(entries, comp)
        qs = search_queries(keys)
        got = DI.handle_hits(idx, qs)
        for q, g in zip(qs, got):
            o = orc.disk_index_search(idx, q, 4096)
            if o[0] != 0:
                assert g[0] == o[0], (comp, r, q, g, o)
            else:
                assert g == o, (comp, r, q, g, o)
        if planted:
            assert any(g[0] == L.RIO_ERR_PROTO for g in got)
        else:  # (the reference's own search misses a key now and then on a compressed file: the oracle decides)
            assert sum(1 for g in got[:len(keys)] if g[0] == 0 and g[2]) > len(keys) * 3 // 4


# ---- end to end ------------------------------------------------------------------------------------------------
def test_table_of_non_canonical_index_records(tmp_path):
    import sstables as S
    from sstables.writer import crc64_iso
    from test_gpu_sstable import check_against_oracle, write_triples

    items = [(be(i) + (b"", b"+" * 13, b"#" * 33)[i % 3], be(i) * (i % 50)) for i in range(300)]
    tri = [(k, v, crc64_iso(v)) for k, v in items]
    base = str(tmp_path / "t")
    seen = []

    def tamper(i, e, off):
        seen.append(W.index_entry_model(e) == (tri[i][0], off, tri[i][2]))
        rec = W.decorated(tri[i][0], off, tri[i][2], i)
        assert rec != e and W.index_entry_model(rec) == (tri[i][0], off, tri[i][2])
        return rec

    write_triples(base, tri, tamper=tamper)
    assert len(seen) == 300 and all(seen)
    o, r = check_against_oracle(base)
    assert r is not None and o["first_bad"] is None and o["unplaced"] is None and o["bad_proto"] is None
    for k, v in items:
        assert r.Contains(k) == (True, None)
        assert r.Get(k) == (v, None)
    # _dec_repeated gives an earlier key first: the entry answers to the last one only
    earlier = b"an earlier key, longer than the last"
    assert any(earlier in W.decorated(k, 1, 2, i) for i, (k, _) in enumerate(items))
    assert r.Contains(earlier) == (False, None) and r.Get(earlier)[1] is S.NotFound
