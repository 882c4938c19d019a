"""Plain Python model of SSTableMerger.Merge / MergeCompact (sstables/sstable_merger.go:36-169) with the
reference's two reducers (super_sstable_reader.go:107-131): the expectation of the compaction tests.
Python's bytes order is bytes.Compare's (lexicographic, unsigned, a proper prefix first)."""


def reduce_latest_wins(key, values, context):
    """ScanReduceLatestWins, super_sstable_reader.go:109-121, line by line."""
    max_ctx = 0
    max_ctx_index = 0
    for i, x in enumerate(context):
        if x > max_ctx:
            max_ctx = x
            max_ctx_index = i
    return key, values[max_ctx_index]


def reduce_latest_wins_skip_tombstones(key, values, context):
    """ScanReduceLatestWinsSkipTombstones, super_sstable_reader.go:125-131 (len(nil) == 0 in Go)."""
    key, val = reduce_latest_wins(key, values, context)
    if val is None or len(val) == 0:
        return None, None
    return key, val


class DuplicateKey(Exception):
    """SSTableStreamWriter.WriteNext: "the same key cannot be written more than once"."""


def _groups(tables):
    """key -> (values, contexts) in the order the priority queue pops equal keys: by table position."""
    g = {}
    for ctx, items in enumerate(tables):
        for k, v in items:
            vals, ctxs = g.setdefault(bytes(k), ([], []))
            vals.append(v)
            ctxs.append(ctx)
    return sorted(g.items())


def merge_all(tables):
    """Merge: every entry in (key, table) order; a repeated key is the writer's error."""
    out = []
    for k, (vals, _) in _groups(tables):
        if len(vals) > 1:
            raise DuplicateKey(k)
        out.append((k, vals[0]))
    return out


def merge_compact(tables, reduce):
    """MergeCompactIterator.Next (sstable_merger.go:79-118): a group is written when both the reduced key
    and the reduced value are non-nil."""
    out = []
    for k, (vals, ctxs) in _groups(tables):
        kr, vr = reduce(k, vals, ctxs)
        if kr is not None and vr is not None:
            out.append((kr, vr))
    return out


def check_reducer(latest_wins, skip_tombstones):
    """The assertions of TestScanReduceFunc / TestScanReduceLatestWinsWithTombstonesFunc
    (super_sstable_reader_test.go:282-324), transcribed."""
    expected_key = bytes([0])
    values = [bytes([0]), bytes([1]), bytes([2]), bytes([3])]
    for f in (latest_wins, skip_tombstones):
        k, v = f(expected_key, values, [3, 2, 1, 0])
        assert k == expected_key and v is values[0]
        k, v = f(expected_key, values, [0, 2, 1, 0])
        assert k == expected_key and v is values[1]
        k, v = f(expected_key, values, [0, 0, 0, 0])
        assert k == expected_key and v is values[0]
    # tombstone case: the latest value is empty
    values = [b"", bytes([1]), bytes([2]), bytes([3])]
    k, v = latest_wins(expected_key, values, [1, 0, 0, 0])
    assert k == expected_key and v is values[0] and v is not None
    k, v = skip_tombstones(expected_key, values, [1, 0, 0, 0])
    assert k is None and v is None
