"""A plain transcription of the reference's sequential write path, with no library calls: the memstore's size
estimate (memstore/memstore.go:119-183 through simpledb/rw_memstore.go:48-63) and the DB's loop of PutBytes /
DeleteBytes with its rotations (simpledb/db.go:256-347, flush.go:32-108, recovery.go:208-277). An op is (key, value)
with value None for a delete. The yardstick of tests/test_db_write_host.py, test_gpu_mem_size.py and test_gpu_db.py."""
import struct

U64 = (1 << 64) - 1
NONE = U64


def f32(x: float) -> float:
    return struct.unpack("f", struct.pack("f", x))[0]


def u64_to_f32(n: int) -> float:
    """Go's float32(uint64): round to nearest, ties to even, worked out on the integer (no double in between)."""
    if n < 1 << 24:
        return float(n)
    shift = n.bit_length() - 24
    q, r, half = n >> shift, n & ((1 << shift) - 1), 1 << (shift - 1)
    if r > half or (r == half and q & 1):
        q += 1
    return float(q << shift)  # at most 25 significant bits: exact as a double


def estimate(raw_size: int) -> int:
    """uint64(1.15 * float32(m.estimatedSize)) (memstore.go:182). The double product of two float32 values is exact,
    so f32() rounds once, as the float32 multiply does. A product of 2^64 and more saturates (the device's rule)."""
    return min(int(f32(f32(1.15) * u64_to_f32(raw_size))), U64)


class ModelMemStore:
    """RWMemstore over a fresh write store: a dict from key to its latest value (None: tombstoned) and estimatedSize."""

    def __init__(self, latest=None, size: int = 0):
        self.latest = dict(latest or {})
        self.size = size & U64

    def upsert(self, key: bytes, value: bytes):
        if key in self.latest:  # memstore.go:129-135: a tombstone's previous length is 0
            prev = self.latest[key]
            self.size = (self.size - (0 if prev is None else len(prev)) + len(value)) & U64
        else:  # :137-138
            self.size = (self.size + len(key) + len(value)) & U64
        self.latest[key] = value

    def delete(self, key: bytes):
        """RWMemstore.Delete: writeStore.Delete, and Tombstone on its KeyNotFound."""
        if key in self.latest:  # memstore.go:158-159
            prev = self.latest[key]
            self.size = (self.size - (0 if prev is None else len(prev))) & U64
        else:  # :172-175
            self.size = (self.size + len(key)) & U64
        self.latest[key] = None

    def apply(self, op):
        key, value = op
        if value is None:
            self.delete(key)
        else:
            self.upsert(key, value)

    def estimated(self) -> int:
        return estimate(self.size)


def scan(store: ModelMemStore, ops, max_size: int):
    """What rio_mem_size_scan reports for `ops` over `store` (which is left unchanged): (sizes after every op, cut,
    size at the cut or at the end). The cut is the first put after which the estimate passes max_size."""
    m = ModelMemStore(store.latest, store.size)
    sizes, cut = [], NONE
    for i, op in enumerate(ops):
        m.apply(op)
        sizes.append(m.size)
        if cut == NONE and op[1] is not None and m.estimated() > max_size:
            cut = i
    last = sizes[cut] if cut != NONE else (sizes[-1] if sizes else store.size)
    return sizes, cut, last


WAL_NAME = "%06d.wal"
TABLE_NAME = "sstable_%015d"


class ModelDB:
    """The directory a DB leaves: `tables` = [(generation, dict)] oldest first, `wal` = {file name: [ops]}. The WAL's
    own size limit (100 x the memstore's) is taken as never reached: max_wal_bytes lets a test check that."""

    def __init__(self, max_size: int):
        self.max_size = max_size
        self.tables, self.generation = [], 0
        self.max_wal_bytes = 0  # the most key and value bytes any WAL file held, removed ones included
        self._open_wal()

    def _open_wal(self):
        self.mem = ModelMemStore()
        self.wal = {WAL_NAME % 0: []}
        self.wal_number = 0

    def _rotate_and_flush(self):
        rotated = WAL_NAME % self.wal_number
        self.max_wal_bytes = max(self.max_wal_bytes, self.raw_wal_bytes())
        self.wal_number += 1
        self.wal[WAL_NAME % self.wal_number] = []
        if not self.mem.latest:  # flush.go:37-40: nothing to write, the WAL file stays
            return
        self.generation += 1
        self.tables.append((self.generation, dict(self.mem.latest)))
        del self.wal[rotated]
        self.mem = ModelMemStore()

    def apply(self, ops):
        for key, value in ops:
            self.wal[WAL_NAME % self.wal_number].append((key, value))
            self.mem.apply((key, value))
            if value is not None and self.mem.estimated() > self.max_size:  # db.go:299; no check in DeleteBytes
                self._rotate_and_flush()

    def close(self):
        self._rotate_and_flush()

    def reopen(self):
        """Open over the directory as it stands: every WAL record replayed (Upsert / Tombstone) into one table of
        the next generation, then a fresh WAL directory (recovery.go:208-277)."""
        m = ModelMemStore()
        for name in sorted(self.wal):
            for op in self.wal[name]:
                m.apply(op)
        if m.latest:
            self.generation += 1
            self.tables.append((self.generation, dict(m.latest)))
        self._open_wal()

    def get(self, key: bytes):
        """db.GetBytes: the value or None (ErrNotFound)."""
        if key in self.mem.latest:
            return self.mem.latest[key]
        for _, t in reversed(self.tables):
            if key in t:
                return t[key] or None  # a nil or empty table value is not found (db.go:219-221)
        return None

    def raw_wal_bytes(self) -> int:
        return max((sum(len(k) + len(v or b"") + 8 for k, v in ops) for ops in self.wal.values()), default=0)
