"""The reader's decoded index and SeekNext map, seen as such (GPU).

Every other ReadAtI test compares an answer with the oracle, and an answer is the same whether the map
(k_count91 .. k_seek_jump, csrc/rio_seek.hip) or the single-record kernels gave it. Here
rio_reader_index_info shows the map itself: for every file of tests/seek_map_model.py's families the
index is built (n_records is the oracle's record count), P is every 0x91 offset and R is the model's
end of the walk from it, exactly. Then SeekNext through the C ABI, from every offset of the small files
and around the sampled positions of the large ones, equals the oracle's; and one gzip index.rio of more
than 1024 segments is searched through k_index_search_view over the same kind of map.
"""
import ctypes
import random
import struct

import numpy as np
import pytest

import corpus
import seek_map_model as M
from recordio import NewMemoryMappedReaderWithPath
from recordio import _lib as L

pytestmark = pytest.mark.gpu
NAMES = [x for x in M.all_names() if x[1] not in ("end_header_only", "end_empty")]
SMALL = 16 << 10  # files below it are sought from every offset


def _open(tmp_path, raw):
    p = tmp_path / "f.rio"
    p.write_bytes(raw)
    r, err = NewMemoryMappedReaderWithPath(str(p))
    assert err is None
    return r


def _seek(r, off):
    data, n, nil, ro = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_int(), ctypes.c_uint64()
    rc = L.lib().rio_reader_seek_next(r._h, off, ctypes.byref(ro), ctypes.byref(data), ctypes.byref(n),
                                      ctypes.byref(nil))
    rec = None
    if rc == 0 and not nil.value:
        rec = ctypes.string_at(data.value, n.value) if n.value else b""
    return rc, (ro.value if rc == 0 else None), rec


def _want(raw, off, seek_len=4096):
    st, ro, rec = M.seek_next(raw, off, seek_len)
    return st, (ro if st == 0 else None), rec


def _offsets(fam, name, raw, P):
    if len(raw) < SMALL and fam not in M.LARGE:  # (`segments` has small files too: they hold one record, and a walk
        return range(len(raw) + 2)               # that runs to the file end is a one-thread scan of the rest of it)
    ks = M.sample(fam, name)
    ks = ks[::max(1, len(ks) * 3 // 2000)]  # about 2000 oracle calls at the most
    return sorted({int(P[k]) + d for k in ks for d in (-1, 0, 1)})


@pytest.mark.parametrize("fam,name", NAMES, ids=[n for _, n in NAMES])
def test_index_is_built_and_equals_the_model(fam, name, tmp_path):
    raw, rec_off, P, R, _ = M.solved(fam, name)
    r = _open(tmp_path, raw)
    assert r.Open() is None
    n, gP, gR = r.index_info()
    assert n == len(rec_off) and n != 0, (n, len(rec_off))
    m = min(gP.size, P.size)
    assert gP.size == P.size and np.array_equal(gP, P), (gP.size, P.size, np.flatnonzero(gP[:m] != P[:m])[:1])
    bad = np.flatnonzero(gR != R)
    assert bad.size == 0, (f"{bad.size} of {R.size} ends differ, the first at k = {int(bad[0])}, offset {int(P[bad[0]])}: "
                           f"device {int(gR[bad[0]])}, model {int(R[bad[0]])}")
    assert L.RIO_SEEK_END_OTHER == M.OTHER and L.RIO_SEEK_END_EOF == M.EOF
    seek_lens = (4096, 4) if fam == "boundaries" else (4096,)
    for seek_len in seek_lens:
        r.seekLen = seek_len
        bad = [(off, g, w[:2]) for off in _offsets(fam, name, raw, P)
               if (g := _seek(r, off)) != (w := _want(raw, off, seek_len))]
        assert not bad, (seek_len, len(bad), [(o, g[:2], w) for o, g, w in bad[:5]])
    r.Close()


def test_header_only_and_empty_files_have_no_index(tmp_path):
    """A file of the 8 header bytes decodes to no record: n_records and K are 0, and every SeekNext is
    the single-record kernel's, with the oracle's status. An empty file does not open (the oracle's
    status for it), so there is no index to show."""
    raw = M.solved("ends", "end_header_only")[0]
    r = _open(tmp_path, raw)
    assert r.Open() is None
    n, gP, gR = r.index_info()
    assert (n, gP.size, gR.size) == (0, 0, 0)
    for off in range(len(raw) + 2):
        assert _seek(r, off) == _want(raw, off), off
    r.Close()
    assert r.index_info() is None  # closed: RIO_ERR_STATE
    r = _open(tmp_path, b"")
    st = M.seek_next(b"", 0)[0]
    assert st == L.RIO_ERR_SHORT_FILE_HEADER and L.lib().rio_reader_open(r._h) == st
    assert r.index_info() is None and _seek(r, 0)[0] == L.RIO_ERR_STATE


def test_index_info_refuses_what_its_neighbours_refuse(tmp_path):
    from recordio import NewFileReaderWithPath

    p = tmp_path / "f.rio"
    p.write_bytes(M.solved("tails", "tail_mod3")[0])
    info = L.ReaderIndexInfo()
    assert L.lib().rio_reader_index_info(None, ctypes.byref(info)) == L.RIO_ERR_ARG
    r, _ = NewMemoryMappedReaderWithPath(str(p))
    assert L.lib().rio_reader_index_info(r._h, None) == L.RIO_ERR_ARG
    assert L.lib().rio_reader_index_info(r._h, ctypes.byref(info)) == L.RIO_ERR_STATE  # not opened yet
    f, _ = NewFileReaderWithPath(str(p))
    assert f.Open() is None
    assert L.lib().rio_reader_index_info(f._h, ctypes.byref(info)) == L.RIO_ERR_STATE  # a FILE-mode reader
    f.Close()


def test_compressed_index_over_a_map_of_more_than_1024_segments():
    """A gzip index.rio of stored (level 0) members, so that the keys' bytes stand in the file as they
    are: 4000-byte keys that hold the `chains` runs of L <= 17 behind a sortable prefix, 1100 of them.
    rio_index_open decodes it and builds the map (k_scan_segs with per = 2); every probe of
    k_index_search_view is a lookup in P / R. Hits equal the oracle's binarySearch on the same bytes
    for every stored key and as many absent ones."""
    from sstables.proto import encode_index_entry

    rng = random.Random(91)
    fill = np.random.default_rng(91).integers(0, 256, size=1100 * 4000, dtype=np.uint8).tobytes()
    runs = [n for Lr in M.CHAIN_GROUPS["small"] for n in (2 * Lr, 2 * Lr + 1)]
    keys = [struct.pack(">I", 2 * i) + b"\x91" * runs[i % len(runs)] + fill[4000 * i:4000 * (i + 1) - 4 - runs[i % len(runs)]]
            for i in range(1100)]
    entries = [encode_index_entry(k, 8 + 4100 * i, 7 * i + 1) for i, k in enumerate(keys)]
    idx = corpus.gz_file([(len(e), corpus.gzip_member(e, 0)) for e in entries])
    assert (len(idx) + M.SEG - 1) // M.SEG > 1024 and b"\x91" * 35 in idx
    absent = [b""] + [struct.pack(">I", 2 * i + 1) + fill[i:i + rng.randrange(0, 40)] for i in range(1099)]
    qs = keys + absent
    h = ctypes.c_void_p()
    assert L.lib().rio_index_open(L.default_ctx(0), idx, len(idx), ctypes.byref(h)) == 0
    try:
        off = np.zeros(len(qs) + 1, dtype=np.uint64)
        np.cumsum([len(q) for q in qs], out=off[1:])
        hits = (L.IndexHit * len(qs))()
        assert L.lib().rio_index_search(h, b"".join(qs), off.ctypes.data, len(qs), hits) == 0
        got = [(x.status, x.offset, bool(x.found), x.value_offset, x.checksum) for x in hits]
    finally:
        L.lib().rio_index_free(h)
    bad = [(i, g, o) for i, (q, g) in enumerate(zip(qs, got))
           if (g[:1] if (o := M.disk_index_search(idx, q))[0] else g) != (o[:1] if o[0] else o)]
    assert not bad, (len(bad), bad[:3])
    assert all(g[2] for g in got[:len(keys)]) and not any(g[2] for g in got[len(keys):])
