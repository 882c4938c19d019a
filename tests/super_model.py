"""Plain Python model of SuperSSTableReader (sstables/super_sstable_reader.go:11-182): the expectation of the
stack tests. A stack is a list of tables, oldest first; a table is a dict key -> value, None for a nil value.
Python's bytes order is bytes.Compare's (lexicographic, unsigned, a proper prefix first)."""

NOT_FOUND = object()


class Stack:
    def __init__(self, tables):
        self.tables = [{bytes(k): v for k, v in (t.items() if isinstance(t, dict) else t)} for t in tables]

    def get(self, key):
        """Get (:34-49): the newest table that holds the key answers, a nil or empty value too; NOT_FOUND."""
        key = bytes(key)
        for t in reversed(self.tables):
            if key in t:
                return t[key]
        return NOT_FOUND

    def contains(self, key) -> bool:
        """Contains (:18-32) of tables without filters, or whose filters hold every key of their table."""
        return any(bytes(key) in t for t in self.tables)

    def source(self, key):
        """(table, position of the key among the table's sorted keys) of the newest table holding it, or None."""
        key = bytes(key)
        for i in range(len(self.tables) - 1, -1, -1):
            if key in self.tables[i]:
                return i, sorted(self.tables[i]).index(key)
        return None

    def scan(self, lo=None, hi=None):
        """Scan / ScanStartingAt(lo) / ScanRange(lo, hi) (:51-105): the sorted union of the keys in [lo, hi], both
        ends inclusive, each with its newest value; a key whose newest value is nil is dropped, an empty value
        stays (MergeCompactIterator with ScanReduceLatestWins, sstable_merger.go:79-118)."""
        out = []
        for k in sorted(set().union(*self.tables) if self.tables else ()):
            if (lo is not None and k < lo) or (hi is not None and k > hi):
                continue
            v = self.get(k)
            if v is not None:
                out.append((k, v))
        return out


def metadata(metas):
    """MetaData (:140-169) as written: (numRecords, dataBytes, indexBytes, totalBytes, version, minKey, maxKey)
    from a list of the same tuples, one per reader. MinKey and MaxKey are both replaced when the running value
    compares LOWER, so both end as the largest of the readers' values (nil compares as the empty key)."""
    num = data = index = total = version = 0
    min_key = max_key = b""
    for n, d, i, t, ver, lo, hi in metas:
        num, data, index, total, version = num + n, data + d, index + i, total + t, ver
        if min_key < (lo or b""):
            min_key = lo
        if max_key < (hi or b""):
            max_key = hi
    return num, data, index, total, version, min_key, max_key
