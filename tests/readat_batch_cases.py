"""Files for the batched ReadNextAt tests (rio_device_read_at_plan / _copy, rio_reader_read_next_at_batch).

Builders only: nothing here decodes. The oracle's read_next_at (tests/oracle_py.py) is the checker of every
offset; tests/test_readat_batch_host.py proves on the CPU that each family reaches the status classes it is
named for, tests/test_gpu_readat_batch.py runs them on the device.

  sweep_files()    per (version 1..4) x (none, snappy, gzip, lzw) two files of at most 4 KiB: "tail" (an empty
                   record, a nil one from v3 on, a record whose header CRC is damaged in v4, 24 zero bytes behind the
                   last record) and "cut" (the same records, the last payload truncated)
  snappy_forms()   one Snappy v4 file: the element forms the wave decoder (coop_record) tells apart
  snappy_corrupt() one Snappy v4 file: four streams that do not decode, each between two good records
  plain_lengths()  one uncompressed v4 file: lengths around kLongItem and the 16-byte store edges
"""
import random
import struct

import corpus
import oracle_py as orc
import snappy_streams as ss

NONE, GZIP, SNAPPY, LZW = 0, 1, 2, 3
CODECS = {"none": NONE, "snappy": SNAPPY, "gzip": GZIP, "lzw": LZW}
K_COOP_RING = 1024  # kCoopRing, csrc/rio_snappy.hip: copies reaching further back read the output arena
K_LONG_ITEM = 1024  # kLongItem, csrc/rio_seg_copy.h


def _sweep_records(version):
    recs = [b"hello world " * 5, b"", bytes(range(40)), b"\x91\x8d\x4c\x00\x05\x05" + b"abc" * 4, b"z" * 100,
            b"the last record's payload\x91\x8d\x4c\x00xyz"]  # cut by 3 bytes, the file ends in a header's first bytes
    if version >= 3:
        recs.insert(2, None)
    return recs


def _damage_crc(img: bytearray, rec_off: int):
    """Flip the lowest bit of a v4 header's CRC varint (its first byte keeps its continuation bit)."""
    p = rec_off + 4
    for _ in range(2):  # u, c
        while img[p] & 0x80:
            p += 1
        p += 1
    img[p] ^= 1


def _gzip_image(recs, version):
    """(image, record offsets): every payload one gzip member."""
    out, offs = bytearray(corpus.file_header(version, GZIP)), []
    for r in recs:
        offs.append(len(out))
        if r is None:
            out += corpus.header_for(version, 0, 0, nil=True)
        else:
            pay = corpus.gzip_member(r)
            out += corpus.header_for(version, len(r), len(pay)) + pay
    return out, offs


def sweep_files():
    """[(name, image)]: 32 files."""
    out = []
    for cname, comp in CODECS.items():
        for version in (1, 2, 3, 4):
            recs = _sweep_records(version)
            if comp == GZIP:
                img, offs = _gzip_image(recs, version)
            else:
                v4, offs = orc.encode_file(recs, comp)
                img = bytearray(v4 if version == 4 else corpus.to_version(v4, version))
            if version == 4:
                _damage_crc(img, offs[-2])
            assert len(img) + 24 <= 4096
            out.append((f"{cname}_v{version}_tail", bytes(img) + b"\0" * 24))
            out.append((f"{cname}_v{version}_cut", bytes(img[:-3])))
    return out


def _stream(build) -> ss.Stream:
    st = ss.Stream()
    build(st)
    return st


def snappy_forms(seed=5):
    """(image, [decoded record]) of a Snappy v4 file, one record per form."""
    rng = random.Random(seed)
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))  # noqa: E731

    def lit_lengths(st):  # literal lengths in the tag, in 1, 2, 3 and 4 bytes
        for n, tag in ((7, None), (60, None), (61, None), (256, None), (257, None), (5, 62), (5, 63)):
            st.literal(rb(n), tag)

    def copy_widths(st):  # tag 1 (11-bit offset), tag 2 (16-bit), tag 3 (32-bit)
        st.literal(rb(300))
        st.copy(7, 5)
        st.copy(290, 30)
        st.copy4(33, 9)

    def overlap(st):  # offset 1: every byte the one before it
        st.literal(rb(3))
        st.copy(1, 64)
        st.copy(1, 5)
        st.copy(2, 37)

    def far(st):  # further back than the history ring: read from the arena
        st.literal(rb(K_COOP_RING + 476))
        st.copy(K_COOP_RING + 1, 64)
        st.copy(K_COOP_RING + 300, 33)
        st.copy(len(st.out), 17)  # the record's first byte

    def many_elements(st):  # more than 64 elements: several rounds by the element count
        st.literal(rb(9))
        for i in range(150):
            if i % 3:
                st.copy(1 + i % 9, 4 + i % 7)
            else:
                st.literal(rb(1 + i % 5))

    def long_stream(st):  # more than 256 stream bytes between element starts: several parse windows
        for _ in range(5):
            st.literal(rb(700))
            st.copy(650, 64)

    builds = [lit_lengths, copy_widths, overlap, far, many_elements, long_stream]
    streams = [_stream(b) for b in builds]
    recs = [bytes(s.out) for s in streams]
    parts = [corpus.file_header(4, SNAPPY)] + [ss.frame(s.payload()) for s in streams]
    parts.append(ss.frame(b"\x00"))  # decoded length 0, not nil
    recs.append(b"")
    assert any(len(s.els) > 256 for s in streams) and max(len(r) for r in recs) > K_COOP_RING
    return b"".join(parts), recs


def snappy_corrupt(seed=6):
    """(image, [decoded record, or None for a stream that does not decode]): good, bad, good, bad, ..."""
    rng = random.Random(seed)
    els = ss.lit(bytes(rng.randrange(256) for _ in range(20)))
    bad = [
        ss.reach_back(rng)[0],         # a copy offset beyond what has been produced
        ss.lit_past_stream(rng)[0],    # a literal running past the stream
        ss.long_of_preamble(rng)[0],   # output overflowing the preamble
        corpus.uvarint(22 * len(els) + 65) + els,  # a preamble above 22 x the element bytes + 64
    ]
    parts, recs = [corpus.file_header(4, SNAPPY)], []
    for i in range(len(bad) + 1):
        st = ss.Stream()
        st.literal(bytes(rng.randrange(256) for _ in range(90 + 40 * i)))
        st.copy(30 + i, 50)
        parts.append(ss.frame(st.payload()))
        recs.append(bytes(st.out))
        if i < len(bad):
            parts.append(ss.frame(bad[i]))
            recs.append(None)
    return b"".join(parts), recs


PLAIN_LENGTHS = (0, 1, 15, 16, 17, K_LONG_ITEM - 1, K_LONG_ITEM, K_LONG_ITEM + 1, 5000)


def plain_lengths(seed=7):
    """(image, records) of an uncompressed v4 file."""
    rng = random.Random(seed)
    recs = [bytes(rng.randrange(256) for _ in range(n)) for n in PLAIN_LENGTHS]
    return orc.encode_file(recs, NONE)[0], recs


def record_starts(img: bytes):
    """The offsets of the records a v4 file of valid headers holds, in file order (header walk, no decode)."""
    comp = struct.unpack_from("<I", img, 4)[0]
    p, out = 8, []
    while p < len(img):
        out.append(p)
        nil = img[p + 3] == 1
        q, vals = p + 4, []
        for _ in range(3):
            v = s = 0
            while True:
                c = img[q]
                q += 1
                v |= (c & 0x7F) << s
                s += 7
                if c < 0x80:
                    break
            vals.append(v)
        p = q + (0 if nil else (vals[1] if comp else vals[0]))
    return out
