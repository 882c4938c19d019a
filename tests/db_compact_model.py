"""A plain transcription of the reference's compaction, with no library calls, over db_write_model.ModelDB: floodFill
and candidateTablesForCompaction (simpledb/sstable_manager.go:115-185), and what executeCompaction followed by
reflectCompactionResult (compaction.go:57-146, sstable_manager.go:24-85) leaves: the selected run merged, latest wins,
nil and empty values dropped (ScanReduceLatestWinsSkipTombstones), in the place of the first selected generation. The
yardstick of tests/test_db_compact_host.py and test_gpu_db_compact.py."""
import db_write_model as wm

DEFAULT_MAX_SIZE = 5 * 1024 * 1024 * 1024
DEFAULT_RATIO = wm.f32(0.2)


def flood_fill(a):
    """floodFill, loop for loop (sstable_manager.go:158-185)."""
    a = list(a)
    i = 0
    while i < len(a):
        if a[i]:
            j = i + 1
            found = False
            while j < len(a):
                if a[j]:
                    for x in range(i, j + 1):
                        a[x] = True
                    i = j - 1
                    found = True
                    break
                j += 1
            if not found and j == len(a):
                return a
        i += 1
    return a


def selected(total_bytes: int, num_records: int, null_values: int, max_size: int, ratio: float) -> bool:
    """One table's own selection (sstable_manager.go:121-125), the ratio in float32 as Go computes it."""
    s = total_bytes < max_size
    if num_records > 0:
        s = s or wm.f32(wm.u64_to_f32(null_values) / wm.u64_to_f32(num_records)) >= wm.f32(ratio)
    return s


def candidates(tables, max_size: int, ratio: float):
    """`tables` = [(name, totalBytes, numRecords, nullValues)] oldest first -> (selected names, sum of numRecords)."""
    sel = flood_fill([selected(tb, n, nulls, max_size, ratio) for _, tb, n, nulls in tables])
    return [t[0] for t, s in zip(tables, sel) if s], sum(t[2] for t, s in zip(tables, sel) if s)


class ModelCompactDB(wm.ModelDB):
    """ModelDB with one compaction pass after every rotation that added a table (not the one of close) when
    `threshold` is not None, and on demand (compact). A pass the model runs by itself takes every table's totalBytes
    as 0: below any size limit a test sets for such a pass."""

    def __init__(self, max_size: int, threshold=None, compaction_max_size: int = DEFAULT_MAX_SIZE,
                 ratio: float = DEFAULT_RATIO):
        super().__init__(max_size)
        self.threshold, self.compaction_max_size, self.ratio = threshold, compaction_max_size, ratio
        self.closing = False
        self.compactions = []  # (replacement generation, [selected generations]) of every pass that compacted

    def _rotate_and_flush(self):
        before = len(self.tables)
        super()._rotate_and_flush()
        if self.threshold is not None and not self.closing and len(self.tables) > before:
            self.compact({}, self.threshold, self.compaction_max_size, self.ratio)

    def close(self):
        self.closing = True
        super().close()
        self.closing = False

    def reopen(self, repair=None):
        """repair: the arguments of the compact() that repairCompactions finishes before anything else, or None.
        The generation is the highest suffix a table directory carries (recovery.go:150-160): a compaction does not
        touch currentGeneration, so a reopened database may count from further down."""
        if repair is not None:
            self.compact(*repair)
        self.generation = max((g for g, _ in self.tables), default=0)
        super().reopen()
        if self.threshold is not None:  # the pass at the end of Open
            self.compact({}, self.threshold, self.compaction_max_size, self.ratio)

    def compact(self, total_bytes_by_generation, threshold: int, max_size: int, ratio: float):
        """One pass -> the selected generations, or None when no more than `threshold` tables were candidates."""
        rows = [(g, total_bytes_by_generation.get(g, 0), len(t), sum(1 for v in t.values() if v is None))
                for g, t in self.tables]
        gens, _ = candidates(rows, max_size, ratio)
        if len(gens) <= threshold:
            return None
        gens.sort()
        merged = {}
        for g, t in self.tables:  # oldest first: a later table's value replaces an earlier one's
            if g in gens:
                merged.update(t)
        merged = {k: v for k, v in merged.items() if v is not None and len(v) != 0}
        self.tables = [(g, merged if g == gens[0] else t) for g, t in self.tables if g == gens[0] or g not in gens]
        self.compactions.append((gens[0], gens))
        return gens
