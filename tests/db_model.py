"""A plain-Python model of simpledb's read path: a dict per memstore (memstore/memstore.go's point calls), a list of
dict tables (oldest first; None is a nil value) and get_bytes transcribed from simpledb/db.go:197-242 over
simpledb/rw_memstore.go:22-36. No device, no library: what the batched reads are compared with."""

NOT_FOUND = "ErrNotFound"        # db.go:35
KEY_NOT_FOUND = "key not found"  # memstore.go:12
KEY_TOMBSTONED = "key was tombstoned"
TABLE_NOT_FOUND = "table: NotFound"


class ModelStore:
    """The latest state per key: bytes, or None for a tombstone; `ops` is the log in application order."""

    def __init__(self):
        self.latest = {}
        self.ops = []  # (key, value or None)

    def upsert(self, key, value):
        self.latest[key] = value
        self.ops.append((key, value))

    def delete(self, key):
        """MemStore.Delete: KeyNotFound for a key the store never saw, else a tombstone."""
        if key not in self.latest:
            return KEY_NOT_FOUND
        self.tombstone(key)
        return None

    def tombstone(self, key):
        self.latest[key] = None
        self.ops.append((key, None))

    def get(self, key):
        if key not in self.latest:
            return None, KEY_NOT_FOUND
        v = self.latest[key]
        if v is None:
            return None, KEY_TOMBSTONED
        return v, None

    def contains(self, key):
        return self.latest.get(key) is not None

    def source(self, key):
        """The op index of the key's latest op, or None."""
        for i in range(len(self.ops) - 1, -1, -1):
            if self.ops[i][0] == key:
                return i
        return None


def rw_get(write, read, key):
    """rw_memstore.go:22-36."""
    v, err = write.get(key)
    if err is not None:
        if err == KEY_NOT_FOUND and read is not None:
            return read.get(key)
        return None, err
    return v, None


def rw_contains(write, read, key):
    return write.contains(key) or (read is not None and read.contains(key))


def tables_get(tables, key):
    """super_sstable_reader.go:34-49 over dict tables: the newest table that holds the key answers, nil too."""
    for t in reversed(tables or []):
        if key in t:
            return t[key], None
    return None, TABLE_NOT_FOUND


def get_bytes(tables, write, read, key):
    """db.go:197-242, line for line (without the open / closed checks and without table read errors)."""
    sstable_not_found = False
    tab_val, err = tables_get(tables, key)
    if err is not None:
        sstable_not_found = True
    elif tab_val is None or len(tab_val) == 0:
        sstable_not_found = True
    mem_val, err = rw_get(write, read, key)
    if err is not None:
        if err == KEY_NOT_FOUND:
            if sstable_not_found:
                return None, NOT_FOUND
            return tab_val, None
        if err == KEY_TOMBSTONED:
            return None, NOT_FOUND
        return None, err
    return mem_val, None


def mem_source(write, read, key):
    """(store, op) of the memstore op that answers, store 1 = the write store when there are two; or None."""
    stores = [s for s in (read, write) if s is not None]
    for pos in range(len(stores) - 1, -1, -1):
        op = stores[pos].source(key)
        if op is not None:
            return pos, op
    return None


def table_source(tables, key):
    """(table, entry) of the newest table that holds the key, entries in sorted key order; or None."""
    for t in range(len(tables or []) - 1, -1, -1):
        if key in tables[t]:
            return t, sorted(tables[t]).index(key)
    return None
