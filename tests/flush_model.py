"""A plain Python model of MemStore.Flush / FlushWithTombstones (memstore/memstore.go:189-238) for the
flush tests: ops applied to a dict in order, then sorted(items). The expectation table is what the host
writer (sstables.write_sstable, the SSTableStreamWriter mirror) writes for the model's pairs.

An op is (key, value): value None is a tombstone (Delete / Tombstone), b"" an empty non-nil value."""

WITH_TOMBSTONES, SKIP_TOMBSTONES = 0, 1  # RIO_FLUSH_*
FILES = ("data.rio", "index.rio", "meta.pb.bin")


def apply(ops):
    """key -> latest value"""
    state = {}
    for k, v in ops:
        state[bytes(k)] = None if v is None else bytes(v)
    return state


def flush_pairs(ops, mode):
    """Sorted (key, value) pairs of the flushed table: the latest op of every key; without tombstones the keys
    whose latest value is nil are left out (an empty non-nil value stays, memstore.go:229)."""
    items = sorted(apply(ops).items())
    if mode == SKIP_TOMBSTONES:
        items = [(k, v) for k, v in items if v is not None]
    return items


def write_expected(path, ops, mode, comp=2):
    """The expectation table; returns (pairs, its MetaData)."""
    from sstables.writer import write_sstable

    pairs = flush_pairs(ops, mode)
    return pairs, write_sstable(path, pairs, comp)


def fill(store, ops):
    """Apply the ops to a MemStore through its public calls (Upsert / Tombstone)."""
    for k, v in ops:
        err = store.Tombstone(k) if v is None else store.Upsert(k, v)
        assert err is None, err
    return store
