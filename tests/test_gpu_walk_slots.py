"""The 16-byte walk slot (WalkSlot, rio_device.h): one slot per walked record holds its offset inside the chunk,
its header length, its three flag bits and its two lengths, written by three walks (the wave walk k_walk, the lane
walk k_walk_lane, and the serial walk_chunk of the scan's repair) and read by k_place; the gzip / lzw resize
passes rewrite its decoded length. Every file here is decoded under each of them and compared with the oracle
(oracle_py.file_reader_decode_arrays) bit for bit: records that fill a chunk's slots to the last one, the flag
bits beside the longest header, lengths past the packed fields (24 bits, the 32 MiB escape of the stream length,
a claimed 2^32 - 1), a resize through the slot, offsets relative to the largest chunk, and the automatic walk
choice for files of C2's record size."""
import functools

import numpy as np
import pytest

import corpus
import oracle_py as orc
from conftest import STATUS
from gpu_util import assert_same_as_oracle
from gpu_util import decode_with as _decode
from gpu_util import decoder_with_env as _decoder

pytestmark = pytest.mark.gpu

WAVE64 = {"RIO_WALK_LANE": "0", "RIO_CHUNK_BYTES": "64"}
WAVE4K = {"RIO_WALK_LANE": "0", "RIO_CHUNK_BYTES": "4096"}
LANE64 = {"RIO_WALK_LANE": "1", "RIO_LANE_CHUNK_BYTES": "64"}
LANE4K = {"RIO_WALK_LANE": "1", "RIO_LANE_CHUNK_BYTES": "4096"}
FRAMINGS = [pytest.param(e, id=i) for i, e in (("wave64", WAVE64), ("wave4096", WAVE4K), ("lane64", LANE64),
                                               ("lane4096", LANE4K))]
# the serial repair writes its slots under either walk: the files made by `embedded` run under both at 4 KiB
REPAIR_FRAMINGS = [pytest.param(e, id=i) for i, e in (("wave4096", WAVE4K), ("lane4096", LANE4K))]


_oracle = {}


def _same(dec, name, img):
    """The decode of `img` equals the oracle's (computed once per file and left unchanged)."""
    if name not in _oracle:
        _oracle[name] = orc.file_reader_decode_arrays(img)
    g = _decode(dec, img)
    assert_same_as_oracle(g, _oracle[name], name)
    return g


def rec(version, comp, u, payload, nil=False):
    """One record's bytes: the header of `version` claiming u decoded bytes, then the payload as it is."""
    return corpus.header_for(version, u, len(payload) if comp else 0, nil=nil) + payload


def embedded(version, comp, body: bytes) -> bytes:
    """`body` (records of a version / codec, without the file header) behind twelve records whose payloads are
    themselves runs of valid small records of the same file type: a chunk that starts inside one finds an entry
    that is not on the chain, so the scan takes the serial repair, which walks those chunks and the ones after
    them again and rewrites their slots."""
    inner = b"".join(rec(version, comp, 1 + i % 40, b"z" * (1 + i % 40)) for i in range(600))
    outer = b"".join(rec(version, comp, len(inner), inner) + rec(version, comp, 3, b"yyy") for _ in range(12))
    return corpus.file_header(version, comp) + outer + body


def _both(version, comp, body: bytes):
    """(plain file, the same records behind embedded files)"""
    return corpus.file_header(version, comp) + body, embedded(version, comp, body)


# ---- slot density: v2's 5-byte empty records fill every chunk's slots = chunk / 5 + 1 to the last one ----
@functools.lru_cache(None)
def dense_files():
    return _both(2, 0, corpus.header_v2(0, 0) * 3000)


@pytest.mark.parametrize("env", FRAMINGS)
def test_slot_density(env, monkeypatch):
    assert len(dense_files()[0]) == 8 + 5 * 3000
    g = _same(_decoder(monkeypatch, env), "dense", dense_files()[0])
    assert g["n_records"] == 3000 and g["status"] == STATUS["EOF"]


@pytest.mark.parametrize("env", REPAIR_FRAMINGS)
def test_slot_density_after_a_repair(env, monkeypatch):
    g = _same(_decoder(monkeypatch, env), "dense-repair", dense_files()[1])
    assert g["n_repairs"] > 0 and g["n_records"] == 3000 + 24


# ---- flag bits and header length together ----
@functools.lru_cache(None)
def flag_files():
    # v4, uncompressed: nil, empty, normal, then a record whose magic and size varints are padded to ten bytes each
    # and whose CRC takes five: 36 header bytes, the longest the reader accepts (corpus "header_36_exact")
    long_pre = corpus.padded_uvarint(0x130691, 10) + b"\x00" + corpus.padded_uvarint(7, 10) + corpus.padded_uvarint(0, 10)
    long_rec = long_pre + corpus.padded_uvarint(corpus.crc32c(long_pre), 5) + b"payload"
    tail = b"".join(rec(4, 0, n, bytes([65 + n]) * n) for n in range(1, 30))
    flags = rec(4, 0, 0, b"", nil=True) + rec(4, 0, 0, b"") + rec(4, 0, 11, b"hello world") + long_rec + tail
    # gzip: an empty payload is gzip.NewReader's io.EOF (the EOF flag); snappy: a preamble that is no varint (the
    # corrupt flag); each among records that decode
    gz = lambda d: rec(4, 1, len(d), corpus.gzip_member(d))  # noqa: E731
    sn = lambda d: rec(4, 2, len(d), corpus.snappy_encode(d))  # noqa: E731
    text = corpus.text_records(12, 5, 20, 300)
    gzip = b"".join(gz(t) for t in text[:6]) + rec(4, 1, 0, b"") + b"".join(gz(t) for t in text[6:])
    snap = b"".join(sn(t) for t in text[:6]) + rec(4, 2, 160, b"\xff" * 11 + b"abc") + b"".join(sn(t) for t in text[6:])
    return {"flags": _both(4, 0, flags), "gzip-eof": _both(4, 1, gzip), "snappy-corrupt": _both(4, 2, snap)}


FLAG_NAMES = ["flags", "gzip-eof", "snappy-corrupt"]
FLAG_WANT = {"flags": (0, [1, 0, 0, 0]), "gzip-eof": (6, [4]), "snappy-corrupt": (6, [2])}  # first record, its flags on


@pytest.mark.parametrize("name", FLAG_NAMES)
@pytest.mark.parametrize("env", FRAMINGS)
def test_flags_and_header_length(env, name, monkeypatch):
    g = _same(_decoder(monkeypatch, env), name, flag_files()[name][0])
    at, want = FLAG_WANT[name]
    assert g["flags"][at:at + len(want)].tolist() == want and g["status"] == STATUS["EOF"], name
    if name == "flags":
        assert int(g["rec_off"][4] - g["rec_off"][3]) == 36 + 7  # the long header was framed, all 36 bytes of it


@pytest.mark.parametrize("name", FLAG_NAMES)
@pytest.mark.parametrize("env", REPAIR_FRAMINGS)
def test_flags_and_header_length_after_a_repair(env, name, monkeypatch):
    g = _same(_decoder(monkeypatch, env), name + "-repair", flag_files()[name][1])
    at, want = FLAG_WANT[name]
    assert g["n_repairs"] > 0 and g["flags"][24 + at:24 + at + len(want)].tolist() == want, name


# ---- length fields ----
@functools.lru_cache(None)
def length_files():
    rng = np.random.default_rng(3)
    small = [rec(4, 0, n, bytes([48 + n % 10]) * n) for n in (3, 700, 0, 64)]
    big = rng.integers(0, 256, 20 << 20, dtype=np.uint8).tobytes()  # past 24 bits, many chunks
    esc = rng.integers(0, 256, (32 << 20) + 5, dtype=np.uint8).tobytes()  # past the slot's stream field: escaped
    wide = small[0] + small[1] + rec(4, 0, len(big), big) + small[2] + rec(4, 0, len(esc), esc) + small[3] + small[1]
    # a snappy preamble claiming 2^32 - 1 bytes in front of a short stream, among records that decode; and an
    # uncompressed header claiming 2^32 - 1 bytes with a short payload, which ends the file
    sn = lambda d: rec(4, 2, len(d), corpus.snappy_encode(d))  # noqa: E731
    text = corpus.text_records(8, 9, 20, 300)
    claim = corpus.uvarint(0xFFFFFFFF) + b"\x08abc"
    snap = b"".join(sn(t) for t in text[:4]) + rec(4, 2, 0xFFFFFFFF, claim) + b"".join(sn(t) for t in text[4:])
    none = b"".join(small) + rec(4, 0, 0xFFFFFFFF, b"short")
    return {"wide": wide, "snappy-claims-4g": snap, "none-claims-4g": none}


@pytest.mark.parametrize("env", FRAMINGS + [pytest.param({"RIO_WALK_LANE": "0", "RIO_CHUNK_BYTES": str(1 << 26)}, id="wave64M"),
                                            pytest.param({"RIO_WALK_LANE": "1", "RIO_LANE_CHUNK_BYTES": str(1 << 26)}, id="lane64M")])
def test_lengths_past_the_packed_fields(env, monkeypatch):
    """A 20 MiB record (past 24 bits, spanning many chunks) and one of 32 MiB + 5 bytes, whose stream length
    escapes the slot: k_place takes it from the chain's next record, which is the chunk's exit at small chunks
    and the next slot at 64 MiB chunks."""
    img = corpus.file_header(4, 0) + length_files()["wide"]
    g = _same(_decoder(monkeypatch, env), "wide", img)
    assert g["n_records"] == 7 and np.diff(g["out_off"]).tolist() == [3, 700, 20 << 20, 0, (32 << 20) + 5, 64, 700]


@pytest.mark.parametrize("env", REPAIR_FRAMINGS)
def test_lengths_past_the_packed_fields_after_a_repair(env, monkeypatch):
    g = _same(_decoder(monkeypatch, env), "wide-repair", embedded(4, 0, length_files()["wide"]))
    assert g["n_repairs"] > 0 and g["n_records"] == 7 + 24


@pytest.mark.parametrize("name,comp", [("snappy-claims-4g", 2), ("none-claims-4g", 0)])
@pytest.mark.parametrize("env", FRAMINGS)
def test_claimed_length_of_4g(env, name, comp, monkeypatch):
    """The oracle's status and flags decide: the snappy record is corrupt and the file goes on, the uncompressed
    one ends the file inside its payload."""
    g = _same(_decoder(monkeypatch, env), name, corpus.file_header(4, comp) + length_files()[name])
    if comp == 2:
        assert g["flags"][4] == 2 and g["n_records"] == 9
    else:
        assert g["status"] == STATUS["UNEXPECTED_EOF"] and g["n_records"] == 4


@pytest.mark.parametrize("name,comp", [("snappy-claims-4g", 2), ("none-claims-4g", 0)])
@pytest.mark.parametrize("env", REPAIR_FRAMINGS)
def test_claimed_length_of_4g_after_a_repair(env, name, comp, monkeypatch):
    g = _same(_decoder(monkeypatch, env), name + "-repair", embedded(4, comp, length_files()[name]))
    assert g["n_repairs"] > 0


# ---- resize through the slot: the lane walk's slots at chunk 64, their decoded length rewritten by the resize pass ----
def test_gzip_resize_through_the_slot(monkeypatch):
    text = corpus.text_records(9, 21, 200, 900)
    two = text[4]
    pays = [(len(t), corpus.gzip_member(t)) for t in text]
    pays[4] = (len(two), corpus.gzip_members(two, [len(two) // 3]))  # two members: the trailer's ISIZE is the second's
    g = _same(_decoder(monkeypatch, LANE64), "gzip-two-members", corpus.gz_file(pays))
    assert g["n_records"] == 9 and int(g["out_off"][5] - g["out_off"][4]) == len(two) and not g["flags"].any()


def test_lzw_resize_through_the_slot(monkeypatch):
    text = corpus.text_records(9, 22, 200, 900)
    pays = [(len(t), orc.lzw_encode(t)) for t in text]
    pays[3] = (len(text[3]) - 10, pays[3][1])  # the header's u is not the decoded size, in both directions
    pays[6] = (len(text[6]) + 300, pays[6][1])
    g = _same(_decoder(monkeypatch, LANE64), "lzw-u-differs", corpus.lzw_file(pays))
    assert g["n_records"] == 9 and np.diff(g["out_off"]).tolist() == [len(t) for t in text]


# ---- relative offsets at the largest chunk whose slot array (chunk / 5 + 1 slots of 16 bytes) stays under 1 GiB ----
BIG_CHUNK = ((1 << 26) - 2) * 5 // 16 * 16


@pytest.mark.parametrize("walk,knob", [("0", "RIO_CHUNK_BYTES"), ("1", "RIO_LANE_CHUNK_BYTES")], ids=["wave", "lane"])
def test_relative_offsets_at_a_large_chunk(walk, knob, monkeypatch):
    assert (BIG_CHUNK // 5 + 1) * 16 < 1 << 30 <= ((BIG_CHUNK + 16) // 5 + 1) * 16
    recs = [bytes([97 + i]) * (1 + 37 * i) for i in range(10)]
    img = corpus.encode_file(recs, 0)
    g = _same(_decoder(monkeypatch, {"RIO_WALK_LANE": walk, knob: str(BIG_CHUNK)}), "ten-records", img)
    assert g["n_chunks"] == 1 and g["n_records"] == 10


# ---- the automatic walk choice for 512..767-byte records ----
AUTO_LANE_CHUNK = 16384  # rio_ctx.cpp: the lane chunk of the 512..767-byte class


def test_auto_walk_takes_the_lane_walk_for_c2_records(monkeypatch):
    """RIO_WALK_LANE unset, a fresh context: C2 (1 M text-like 1 KiB records, a 561-byte mean in the file, 34 250
    lane chunks of 16 KiB) is framed by the lane walk once the context knows the file's mean, which is from the
    capacity probe of DeviceDecoder.decode on (info.n_chunks is the real decode's): both decodes show the lane
    walk's chunk count, and both equal the oracle."""
    from recordio.device import DeviceDecoder

    for k in ("RIO_WALK_LANE", "RIO_CHUNK_BYTES", "RIO_LANE_CHUNK_BYTES", "RIO_LANE_WALK_MIN"):
        monkeypatch.delenv(k, raising=False)
    dec = DeviceDecoder(0, own_ctx=True)
    img = corpus.generate(1_000_000, 1024, 2, kind=1, seed=1)
    mean = (len(img) - 8) // 1_000_000
    want = (len(img) - 8 + AUTO_LANE_CHUNK - 1) // AUTO_LANE_CHUNK
    assert 512 <= mean < 768 and len(img) // 16384 >= 32768
    first = _same(dec, "c2", img)
    second = _same(dec, "c2", img)
    assert second["n_chunks"] == want and first["n_chunks"] == want
    assert second["n_records"] == 1_000_000 and second["status"] == STATUS["EOF"]
