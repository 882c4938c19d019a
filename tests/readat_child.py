"""Child process of tests/test_gpu_readat_kernel_only.py (needs a GPU).

librio reads RIO_READAT_INDEX_MAX once per process, so the kernel-only path of a reader (no decoded
index, no SeekNext map: what every file that decodes to more than 4 GiB gets) is reached by a fresh
process with the variable set. This one opens the files of its mode, asserts that no index was built
(rio_reader_index_info: n_records == 0), then holds rio_reader_read_next_at and rio_reader_seek_next
to the oracle, and exits 0 after one `ok` line, or 1 after a one-line reason.

  RIO_READAT_INDEX_MAX=0      uncompressed and Snappy files: k_read_at / k_seek_next with
                              snappy_decode_thread, and read_at_impl's grow-and-retry of its output
  RIO_READAT_INDEX_MAX=65536  gzip and lzw files: readat_expand for every record
"""
import ctypes
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(HERE), "go-sstables_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = ((1 << 20) - 1, 1 << 20, (1 << 20) + 1, 3 << 20)  # around and above readat_out's first 1 MiB
OVER_CAP = 70_000  # one record above RIO_READAT_INDEX_MAX=65536: readat_expand applies the same cap


def _compressible(n, seed):
    import corpus

    base = b"".join(corpus.text_records(120, seed, 200, 1500))
    return (base * (n // len(base) + 1))[:n]


def size_records():
    """The four sizes with small records between: a record read after a larger one must be its own."""
    recs = [b"first"]
    for i, n in enumerate(SIZES):
        recs += [_compressible(n, 5 + i), b"small-%d" % i, None if i == 1 else b"s" * (40 + i)]
    return recs


def snappy_forms_file():
    """Every form of tests/snappy_streams.py, valid and invalid, three draws each, in a seeded order."""
    import corpus
    import snappy_streams as S

    rng = random.Random(17)
    recs = [S.frame(S.FORMS[name](rng)[0]) for name in S.ALL for _ in range(3)]
    rng.shuffle(recs)
    return corpus.file_header(4, 2) + b"".join(recs)


def codec_file(comp):
    """gzip (1) / lzw (3): records of 4 to 16 KiB that decode to more than 256 KiB, and among them a nil
    record, a corrupt one, an empty payload, a gzip record of two members, and one of OVER_CAP bytes."""
    import corpus
    import oracle_py as orc

    text = corpus.text_records(34, 23 + comp, 4000, 16000)
    assert sum(len(t) for t in text) >= 256 << 10 and max(len(t) for t in text) <= 16 << 10
    enc = (lambda r: corpus.gzip_member(r)) if comp == 1 else orc.lzw_encode
    items = [(len(r), enc(r)) for r in text]
    items[3] = None
    items[7] = (items[7][0], items[7][1][:len(items[7][1]) // 2])  # cut in the middle: the codec's error
    items[11] = (0, b"")  # gzip: io.EOF, a trial SeekNext passes; lzw: io.ErrUnexpectedEOF
    if comp == 1:
        items[15] = (len(text[15]), corpus.gzip_members(text[15], [len(text[15]) // 2]))
    big = _compressible(OVER_CAP, 31)
    items.insert(20, (len(big), enc(big)))
    return (corpus.gz_file if comp == 1 else corpus.lzw_file)(items), 20


class Reader:
    """An MMAP-mode rio_reader on a context of its own (readat_out starts at 1 MiB in each)."""

    def __init__(self, path):
        from recordio import _lib as L

        self.L, self.lib = L, L.lib()
        self.ctx, self.h = ctypes.c_void_p(), ctypes.c_void_p()
        assert self.lib.rio_ctx_create(0, ctypes.byref(self.ctx)) == 0
        assert self.lib.rio_reader_new_mmap(self.ctx, path.encode(), ctypes.byref(self.h)) == 0
        assert self.lib.rio_reader_open(self.h) == 0

    def n_records(self):
        info = self.L.ReaderIndexInfo()
        assert self.lib.rio_reader_index_info(self.h, ctypes.byref(info)) == 0
        return int(info.n_records), int(info.n_positions)

    def _rec(self, rc, data, n, nil):
        if rc or nil.value:
            return None
        return ctypes.string_at(data.value, n.value) if n.value else b""

    def read_next_at(self, off):
        data, n, nil = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_int()
        rc = self.lib.rio_reader_read_next_at(self.h, off, ctypes.byref(data), ctypes.byref(n), ctypes.byref(nil))
        return rc, self._rec(rc, data, n, nil)

    def seek_next(self, off):
        data, n, nil, ro = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_int(), ctypes.c_uint64()
        rc = self.lib.rio_reader_seek_next(self.h, off, ctypes.byref(ro), ctypes.byref(data), ctypes.byref(n),
                                           ctypes.byref(nil))
        return rc, ro.value, self._rec(rc, data, n, nil)

    def close(self):
        self.lib.rio_reader_free(self.h)
        self.lib.rio_ctx_destroy(self.ctx)


def seeded_offsets(raw, starts, count, seed, heavy=()):
    """`count` offsets: half anywhere in the file, half within 48 bytes before to 8 after a record
    start. In a file with records of a megabyte and more (`heavy`: their numbers) a scan from
    anywhere would mostly cross or decode one of those on a single thread, so there every offset is
    near a start, and only one per heavy record leads to it."""
    rng = random.Random(seed)
    light = [k for k in range(len(starts)) if k not in heavy and k + 1 not in heavy]  # (a few bytes on lies k + 1)
    out = []
    for i in range(count):
        if not heavy and i % 2:
            out.append(rng.randrange(len(raw) + 2))
        else:
            s = starts[rng.choice(light)]
            out.append(max(0, s + rng.randrange(-48, 9)))
    for k in heavy:
        out.append(starts[k] - 1)
    return out


def check(what, raw, heavy=(), over_cap=None, count=300):
    """None, or the first disagreement with the oracle as one line."""
    import tempfile

    import oracle_py as orc
    import seek_map_model as M
    from recordio import _lib as L

    o = orc.file_reader_decode_arrays(raw)
    starts = [int(x) for x in o["rec_off"]]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "f.rio")
        with open(path, "wb") as f:
            f.write(raw)
        r = Reader(path)
        try:
            if r.n_records() != (0, 0):
                return f"{what}: an index was built, n_records / K = {r.n_records()}"
            cap_at = starts[over_cap] if over_cap is not None else None

            def want_at(off):
                return (L.RIO_ERR_CAPACITY, None) if off == cap_at else M.read_next_at(raw, off)

            def want_seek(off):
                st, ro, rec = M.seek_next(raw, off)
                if ro == cap_at and st == 0:
                    return L.RIO_ERR_CAPACITY, ro, None
                return st, ro, rec

            for k, off in enumerate(starts):
                got, want = r.read_next_at(off), want_at(off)
                if got != want:
                    return f"{what}: ReadNextAt at record {k} (offset {off}): {_brief(got)}, want {_brief(want)}"
            for off in seeded_offsets(raw, starts, count, 1, heavy):
                if off in starts:
                    continue
                got, want = r.read_next_at(off), want_at(off)
                if got != want:
                    return f"{what}: ReadNextAt at offset {off}: {_brief(got)}, want {_brief(want)}"
            for off in seeded_offsets(raw, starts, count, 2, heavy) + [len(raw) - 1, len(raw), len(raw) + 1]:
                got, want = r.seek_next(off), want_seek(off)
                if want[0] in (L.RIO_EOF, L.RIO_ERR_INVALID_OFFSET):  # no trial offset to report
                    got, want = (got[0], got[2]), (want[0], want[2])
                if got != want:
                    return f"{what}: SeekNext from offset {off}: {_brief(got)}, want {_brief(want)}"
        finally:
            r.close()
    return None


def _brief(t):
    return tuple(f"<{len(x)} bytes>" if isinstance(x, bytes) and len(x) > 24 else x for x in t)


def main():
    import seek_map_model as M
    from recordio import encode_file

    cap = os.environ.get("RIO_READAT_INDEX_MAX")
    if cap == "0":
        recs = size_records()
        heavy = [k for k, x in enumerate(recs) if x is not None and len(x) >= SIZES[0]]
        jobs = [("snappy forms", snappy_forms_file(), (), None),
                ("ends snappy", M.family("ends")["end_snappy"], (), None),
                ("snappy sizes", bytes(encode_file(recs, 2)), heavy, None),
                ("uncompressed sizes", bytes(encode_file(recs, 0)), heavy, None)]
        count = 300
    elif cap == "65536":
        jobs = [(name, *codec_file(comp)) for name, comp in (("gzip", 1), ("lzw", 3))]
        jobs = [(name, raw, (), over) for name, raw, over in jobs]
        count = 200
    else:
        print(f"FAIL RIO_READAT_INDEX_MAX={cap!r}: this child knows the values 0 and 65536")
        return 1
    for what, raw, heavy, over in jobs:
        err = check(what, raw, heavy, over, count)
        if err:
            print(f"FAIL [RIO_READAT_INDEX_MAX={cap}] {err}")
            return 1
    print(f"ok [RIO_READAT_INDEX_MAX={cap}] {len(jobs)} files")
    return 0


if __name__ == "__main__":
    sys.exit(main())
