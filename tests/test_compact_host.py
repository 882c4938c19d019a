"""Merge-compaction, the parts that need no GPU: the tests' Python model against the reference's own
reducer assertions, argument errors of the new C entry points that return before any device call, and
the IndexEntry length rule against the host encoder."""
import ctypes

import pytest

import compact_model as M
from recordio import _lib as L
from sstables import proto


def test_model_passes_the_reference_reducer_assertions():
    M.check_reducer(M.reduce_latest_wins, M.reduce_latest_wins_skip_tombstones)


def test_exported_reducers_pass_the_reference_reducer_assertions():
    import sstables as S

    M.check_reducer(S.ScanReduceLatestWins, S.ScanReduceLatestWinsSkipTombstones)
    assert S.ScanReduceLatestWins.mode == L.RIO_MERGE_LATEST_WINS
    assert S.ScanReduceLatestWinsSkipTombstones.mode == L.RIO_MERGE_LATEST_WINS_SKIP_TOMBSTONES


def test_model_merge_rules():
    a = [(b"a", b"1"), (b"b", None), (b"c", b""), (b"d", b"4")]
    b = [(b"a", None), (b"b", b"2"), (b"c", b"3"), (b"e", b"")]
    assert M.merge_compact([a, b], M.reduce_latest_wins) == [(b"b", b"2"), (b"c", b"3"), (b"d", b"4"), (b"e", b"")]
    assert M.merge_compact([b, a], M.reduce_latest_wins) == [(b"a", b"1"), (b"c", b""), (b"d", b"4"), (b"e", b"")]
    assert M.merge_compact([b, a], M.reduce_latest_wins_skip_tombstones) == [(b"a", b"1"), (b"d", b"4")]
    assert M.merge_all([a, [(b"aa", None)]]) == [(b"a", b"1"), (b"aa", None), (b"b", None), (b"c", b""), (b"d", b"4")]
    with pytest.raises(M.DuplicateKey):
        M.merge_all([a, b])


def test_merge_argument_errors_return_before_any_device_call():
    lib = L.lib()
    # A context cannot be created without a device, so ctx is a placeholder. It is never read: the three entry
    # points check their arguments before the first read of *ctx (rio_tables.cpp states that order), and every
    # call below is refused on its arguments. The page of zeros keeps a reordering there from reading past it.
    page = ctypes.create_string_buffer(1 << 16)
    ctx = ctypes.addressof(page)
    views = (L.SstView * (L.RIO_MERGE_MAX_TABLES + 1))()
    v, buf = ctypes.addressof(views), ctypes.addressof(ctypes.create_string_buffer(64))
    plan = lib.rio_sst_merge_plan
    assert plan(None, v, 1, L.RIO_MERGE_ALL, buf, buf, buf, None) == L.RIO_ERR_ARG
    assert plan(ctx, None, 1, L.RIO_MERGE_ALL, buf, buf, buf, None) == L.RIO_ERR_ARG
    assert plan(ctx, v, 0, L.RIO_MERGE_ALL, buf, buf, buf, None) == L.RIO_ERR_ARG
    assert plan(ctx, v, L.RIO_MERGE_MAX_TABLES + 1, L.RIO_MERGE_ALL, buf, buf, buf, None) == L.RIO_ERR_ARG
    assert plan(ctx, v, 1, 3, buf, buf, buf, None) == L.RIO_ERR_ARG
    assert plan(ctx, v, 1, L.RIO_MERGE_LATEST_WINS, buf, buf, None, None) == L.RIO_ERR_ARG
    views[0].n = 1  # entries without arrays
    assert plan(ctx, v, 1, L.RIO_MERGE_LATEST_WINS, buf, buf, buf, None) == L.RIO_ERR_ARG
    for f in ("index", "key_off", "key_len", "data", "data_off", "flags", "crc"):
        setattr(views[0], f, buf)
    views[0].n = 1 << L.RIO_MERGE_ENTRY_BITS  # past the packed entry number
    assert plan(ctx, v, 1, L.RIO_MERGE_LATEST_WINS, buf, buf, buf, None) == L.RIO_ERR_UNSUPPORTED
    assert lib.rio_sst_merge_gather(None, buf, buf, 0, buf, buf, 64, buf, buf, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_merge_gather(ctx, buf, buf, 0, buf, None, 64, buf, buf, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_index_encode(None, buf, buf, 0, buf, 64, buf, None) == L.RIO_ERR_ARG
    assert lib.rio_sst_index_encode(ctx, buf, buf, 0, buf, 64, None, None) == L.RIO_ERR_ARG


# every varint width boundary of a uint64: 2^(7k) - 1 and 2^(7k), then the top of the range
_EDGES = sorted({0, 1, (1 << 64) - 1, 1 << 63, (1 << 63) - 1} | {(1 << (7 * k)) - 1 for k in range(1, 10)} |
                {1 << (7 * k) for k in range(1, 10)})


def test_index_entry_length_matches_the_host_encoder():
    lib = L.lib()
    total = n = 0
    for kl in (0, 1, 40, 127, 128, 16383, 16384):
        key = b"k" * kl
        for off in _EDGES:
            for cs in _EDGES:
                want = len(proto.encode_index_entry(key, off, cs))
                assert lib.rio_index_entry_len(kl, off, cs) == want, (kl, off, cs)
                total += want
                n += 1
        assert lib.rio_index_entries_bound(1, kl) >= len(proto.encode_index_entry(key, (1 << 64) - 1, (1 << 64) - 1))
    assert lib.rio_index_entries_bound(n, sum(kl * len(_EDGES) ** 2 for kl in (0, 1, 40, 127, 128, 16383, 16384))) >= total
