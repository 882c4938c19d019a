"""The memstore mirror, the parts that need no GPU: the assertions of memstore/memstore_test.go (every test
that does not flush; those are in test_gpu_memstore_flush.py), the flush tests' Python model against the
oracle's table reader, and the argument errors of rio_sst_flush_plan, which return before any device call."""
import ctypes

import flush_model as FM
import memstore as MS
import oracle_py as orc
import sstables as S
from recordio import _lib as L


def new():
    return MS.NewMemStore()


def test_add_happy_path():  # TestMemStoreAddHappyPath
    m = new()
    assert not m.Contains(b"a")
    val, err = m.Get(b"a")
    assert val is None and err is MS.KeyNotFound
    assert m.Add(b"a", b"aVal") is None
    assert m.Contains(b"a") and not m.IsTombstoned(b"a")
    val, err = m.Get(b"a")
    assert err is None and val == b"aVal"


def test_add_fails_on_nil_key_and_value():  # TestMemStoreAddFailOnNilKeyValue
    m = new()
    err = m.Add(None, None)
    assert err is MS.KeyNil and str(err) == "key was nil"
    err = m.Add(b"a", None)
    assert err is MS.ValueNil and str(err) == "value was nil"
    assert m.Upsert(None, b"x") is MS.KeyNil and m.Upsert(b"a", None) is MS.ValueNil
    assert m.Size() == 0
    assert m.Add(b"", b"") is None  # empty is not nil
    assert m.Get(b"") == (b"", None)


def test_error_texts():  # memstore.go:10-14
    assert [str(e) for e in (MS.KeyAlreadyExists, MS.KeyNotFound, MS.KeyTombstoned, MS.KeyNil, MS.ValueNil)] == [
        "key already exists", "key not found", "key was tombstoned", "key was nil", "value was nil"]


def test_add_fails_on_exist():  # TestMemStoreAddFailsOnExist
    m = new()
    assert m.Add(b"a", b"aVal") is None
    assert m.Add(b"a", b"aVal") is MS.KeyAlreadyExists


def test_upsert_behaves_like_add():  # TestMemStoreUpsertBehavesLikeAdd
    m = new()
    assert m.Upsert(b"a", b"aVal") is None
    assert m.Contains(b"a")
    assert m.Get(b"a") == (b"aVal", None)


def test_upsert_updates_on_exist():  # TestMemStoreUpsertUpdatesOnExist
    m = new()
    assert m.Upsert(b"a", b"aVal") is None
    assert m.Contains(b"a") and m.Get(b"a") == (b"aVal", None)
    assert m.Upsert(b"a", b"aVal2") is None
    assert m.Contains(b"a") and m.Get(b"a") == (b"aVal2", None)


def test_delete_tombstones():  # TestMemStoreDeleteTombstones
    m = new()
    assert m.Upsert(b"a", b"aVal") is None
    assert m.Contains(b"a") and m.Get(b"a") == (b"aVal", None)
    assert m.Delete(b"a") is None
    assert not m.Contains(b"a") and m.IsTombstoned(b"a")
    val, err = m.Get(b"a")
    assert val is None and err is MS.KeyTombstoned


def test_add_tombstoned_key_again():  # TestMemStoreAddTombStonedKeyAgain
    m = new()
    assert m.Upsert(b"a", b"aVal") is None and m.Size() == 1
    assert m.Delete(b"a") is None
    assert not m.Contains(b"a") and m.Size() == 1  # a tombstone keeps its place
    assert m.Add(b"a", b"aVal2") is None
    assert m.Contains(b"a") and m.Size() == 1 and m.Get(b"a") == (b"aVal2", None)


def test_delete_semantics():  # TestMemStoreDeleteSemantics
    m = new()
    assert m.Upsert(b"a", b"aVal") is None and m.Contains(b"a")
    assert m.Delete(b"b") is MS.KeyNotFound
    assert m.DeleteIfExists(b"b") is None
    assert not m.IsTombstoned(b"b") and m.Size() == 1  # no tombstone for a key that was never there
    assert m.DeleteIfExists(b"a") is None
    assert not m.Contains(b"a")
    val, err = m.Get(b"a")
    assert val is None and err is MS.KeyTombstoned


def test_size_estimates():  # TestMemStoreSizeEstimates
    m = new()
    key = bytes(20)
    assert m.Size() == 0
    assert m.Upsert(key, bytes(50)) is None
    assert m.EstimatedSizeInBytes() == 80 and m.Size() == 1
    assert m.Upsert(key, bytes(100)) is None
    assert m.EstimatedSizeInBytes() == 138 and m.Size() == 1
    assert m.Delete(key) is None
    assert m.EstimatedSizeInBytes() == 23 and m.Size() == 1
    assert m.Upsert(key, bytes(200)) is None
    assert m.EstimatedSizeInBytes() == 253 and m.Size() == 1


def _drain(it):
    out = []
    while True:
        k, v, err = it.Next()
        if err is not None:
            assert err is S.Done
            return out
        out.append((k, v))


def test_sstable_iterator_upsert_only():  # TestMemStoreSStableIteratorUpsertOnly
    m = new()
    for p in (b"c", b"a", b"b"):  # the iterator is ordered by key, not by arrival
        assert m.Upsert(p + b"key", p + b"val") is None
    it = m.SStableIterator()
    assert _drain(it) == [(p + b"key", p + b"val") for p in (b"a", b"b", b"c")]
    assert it.Next() == (None, None, S.Done)  # and stays done


def test_sstable_iterator_with_tombstones():  # TestMemStoreSStableIteratorWithTombstones
    m = new()
    for p in (b"a", b"b", b"c"):
        assert m.Upsert(p + b"key", p + b"val") is None
    assert m.Delete(b"bkey") is None
    assert _drain(m.SStableIterator()) == [(b"akey", b"aval"), (b"bkey", None), (b"ckey", b"cval")]


def test_tombstone_existing_key():  # TestMemStoreTombstoneExistingKey
    m = new()
    key = bytes(20)
    assert m.Upsert(key, bytes(50)) is None
    assert m.EstimatedSizeInBytes() == 80 and m.Size() == 1
    assert m.Tombstone(key) is None
    assert m.EstimatedSizeInBytes() == 23 and m.Size() == 1
    assert m.Get(key) == (None, MS.KeyTombstoned)


def test_tombstone_not_existing_key():  # TestMemStoreTombstoneNotExistingKey
    m = new()
    key = bytes(20)
    assert m.Tombstone(key) is None
    assert m.EstimatedSizeInBytes() == 23 and m.Size() == 1
    assert m.Get(key) == (None, MS.KeyTombstoned)


def test_every_mutating_call_is_logged_and_nothing_else():
    """The op log is what the device flush orders: one entry per applied change, in application order, never
    deduplicated; refused calls leave it alone."""
    m = new()
    assert m.Add(b"k", b"1") is None
    assert m.Add(b"k", b"2") is MS.KeyAlreadyExists
    assert m.Upsert(b"k", b"") is None
    assert m.Delete(b"zz") is MS.KeyNotFound and m.DeleteIfExists(b"zz") is None
    assert m.Delete(b"k") is None and m.Tombstone(b"k") is None and m.Tombstone(b"new") is None
    assert m.Upsert(b"k", b"345") is None
    assert bytes(m._keys) == b"kkkknewk" and m._key_off == [0, 1, 2, 3, 4, 7, 8]
    assert bytes(m._values) == b"1345" and m._val_off == [0, 1, 1, 1, 1, 1, 4]
    assert list(m._flags) == [0, 0, 1, 1, 1, 0]
    assert m.Size() == 2 and m._max_key_len == 3


def test_flush_refusals_before_any_device_work(tmp_path):
    m = new()
    assert m.Upsert(b"a", b"1") is None
    assert str(m.Flush()) == "basePath was not supplied"
    for c in (L.COMP_GZIP, L.COMP_LZW, 9):
        err = m.Flush(S.WriteBasePath(str(tmp_path / "t")), S.DataCompressionType(c))
        assert isinstance(err, S.UnsupportedError), err
    assert m.Upsert(b"k" * (L.RIO_FLUSH_MAX_KEY_LEN + 1), b"1") is None
    assert isinstance(m.FlushWithTombstones(S.WriteBasePath(str(tmp_path / "t"))), S.UnsupportedError)
    assert not (tmp_path / "t").exists()


# ---- the flush tests' model ----------------------------------------------------------------------------

_OPS = [(b"b", b"1"), (b"a", b"x"), (b"b", None), (b"c", b""), (b"a\0", b"y"), (b"a", b"z"), (b"d", None),
        (b"d", b"back"), (b"e", b"gone"), (b"e", None), (b"", b"empty key")]


def test_model_rules():
    assert FM.flush_pairs(_OPS, FM.WITH_TOMBSTONES) == [
        (b"", b"empty key"), (b"a", b"z"), (b"a\0", b"y"), (b"b", None), (b"c", b""), (b"d", b"back"), (b"e", None)]
    assert FM.flush_pairs(_OPS, FM.SKIP_TOMBSTONES) == [
        (b"", b"empty key"), (b"a", b"z"), (b"a\0", b"y"), (b"c", b""), (b"d", b"back")]
    assert (FM.WITH_TOMBSTONES, FM.SKIP_TOMBSTONES) == (L.RIO_FLUSH_WITH_TOMBSTONES, L.RIO_FLUSH_SKIP_TOMBSTONES)


def test_model_agrees_with_the_memstore_mirror():
    m = FM.fill(new(), _OPS)
    assert _drain(m.SStableIterator()) == FM.flush_pairs(_OPS, FM.WITH_TOMBSTONES)


def test_expectation_table_reads_back_as_the_model_pairs(tmp_path):
    """The expectation table through the oracle's table reader (test_oracle_sstable.py's)."""
    for mode in (FM.WITH_TOMBSTONES, FM.SKIP_TOMBSTONES):
        for comp in (0, 2):
            base = str(tmp_path / f"t{mode}{comp}")
            pairs, meta = FM.write_expected(base, _OPS, mode, comp)
            o = orc.sstable_oracle(base)
            assert o["first_bad"] is None and o["unplaced"] is None and o["bad_proto"] is None
            assert [e[0] for e in o["entries"]] == [k for k, _ in pairs]
            assert o["values"] == [v for _, v in pairs]
            assert meta.numRecords == len(pairs) and meta.nullValues == sum(v is None for _, v in pairs)
    pairs, meta = FM.write_expected(str(tmp_path / "empty"), [], FM.SKIP_TOMBSTONES)
    assert pairs == [] and meta.numRecords == 0 and orc.sstable_oracle(str(tmp_path / "empty"))["entries"] == []


# ---- rio_sst_flush_plan: argument errors ---------------------------------------------------------------

def test_flush_plan_argument_errors_return_before_any_device_call():
    lib = L.lib()
    # As in test_compact_host.py: no context can be created without a device, so ctx is a placeholder that is
    # never read: the entry point checks its arguments before the first read of *ctx. The page of zeros keeps
    # a reordering there from reading past it.
    page = ctypes.create_string_buffer(1 << 16)
    ctx = ctypes.addressof(page)
    ops = L.OpsView()
    o, buf = ctypes.addressof(ops), ctypes.addressof(ctypes.create_string_buffer(64))
    plan = lib.rio_sst_flush_plan
    WITH, SKIP = L.RIO_FLUSH_WITH_TOMBSTONES, L.RIO_FLUSH_SKIP_TOMBSTONES
    assert plan(None, o, WITH, 8, buf, buf, buf, None) == L.RIO_ERR_ARG
    assert plan(ctx, None, WITH, 8, buf, buf, buf, None) == L.RIO_ERR_ARG
    assert plan(ctx, o, SKIP, 8, buf, buf, None, None) == L.RIO_ERR_ARG
    assert plan(ctx, o, 2, 8, buf, buf, buf, None) == L.RIO_ERR_ARG  # unknown mode
    ops.n = 1  # ops without arrays
    assert plan(ctx, o, SKIP, 8, buf, buf, buf, None) == L.RIO_ERR_ARG
    fields = ("keys", "key_off", "values", "val_off", "flags")
    for missing in fields:
        for f in fields:
            setattr(ops, f, None if f == missing else buf)
        assert plan(ctx, o, SKIP, 8, buf, buf, buf, None) == L.RIO_ERR_ARG, missing
    for f in fields:
        setattr(ops, f, buf)
    assert plan(ctx, o, SKIP, 8, None, buf, buf, None) == L.RIO_ERR_ARG
    assert plan(ctx, o, SKIP, 8, buf, None, buf, None) == L.RIO_ERR_ARG
    assert plan(ctx, o, SKIP, L.RIO_FLUSH_MAX_KEY_LEN + 1, buf, buf, buf, None) == L.RIO_ERR_UNSUPPORTED
    ops.n = (1 << 31) - 1
    assert plan(ctx, o, SKIP, 8, buf, buf, buf, None) == L.RIO_ERR_UNSUPPORTED
    assert lib.rio_sst_flush_stage_ms(None, None, 0) == 0
