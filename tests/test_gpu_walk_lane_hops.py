"""The lane walk's hop (k_walk_lane, RIO_WALK_LANE=1) takes a record's lengths first, loads the next header at the
address they give, and verifies the record under that load; its entry search hands the record it framed to the walk;
v4 files without compression and with snappy run through their own instantiations. Hand-built files around each of those edges: unverified lengths that would be used as an address,
headers at the edges of the entry search's two 128-byte lines, every version and codec, and launch geometries. Every
result is the oracle's: records, offsets, flags, status, status offset and CRC details."""
import random
import struct

import pytest

import corpus
import oracle_py as orc
from conftest import STATUS
from corpus import crc32c, file_header, header_for, header_v4, padded_uvarint, uvarint
from gpu_util import assert_same_as_oracle

pytestmark = pytest.mark.gpu

MAGIC = b"\x91\x8d\x4c"


def _lane_decoder(monkeypatch, chunk):
    from recordio import _lib as L
    from recordio.device import DeviceDecoder

    monkeypatch.setenv("RIO_WALK_LANE", "1")
    monkeypatch.setenv("RIO_LANE_CHUNK_BYTES", str(chunk))
    dec = DeviceDecoder(0, own_ctx=True)  # the context reads the framing knobs when it is created
    assert L.lib().rio_ctx_device(dec.ctx) == 0
    return dec


def _check(dec, name, img):
    from recordio.device import to_device_file

    img = bytes(img)
    o = orc.file_reader_decode_arrays(img)
    d_file, n = to_device_file(img)
    b, info = dec.decode(d_file, n)
    k = info["n_records"]
    g = dict(info, out=b.out[: info["total_out_bytes"]].cpu().numpy(), out_off=b.out_off[: k + 1].cpu().numpy(),
             rec_off=b.rec_off[:k].cpu().numpy(), flags=b.flags[:k].cpu().numpy())
    assert_same_as_oracle(g, o, name)
    return g, o


def _payload(rng, n):
    """n text-like bytes without 0x91: no candidate for the entry search but the ones a test places."""
    return bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz ,.\n") for _ in range(n))


def _record(version, comp, data):
    """One record of `data` as (header, payload) in a file of this version and codec (0 none, 2 snappy)."""
    if comp == 2:
        pay = corpus.snappy_encode(data)
        return header_for(version, len(data), len(pay)), pay
    return header_for(version, len(data), 0), data


def _records_file(version, comp, n, seed, lo=40, hi=1100):
    """(image, record start offsets) of n records of lo..hi payload bytes."""
    rng = random.Random(seed)
    out, offs = bytearray(file_header(version, comp)), []
    for _ in range(n):
        h, pay = _record(version, comp, _payload(rng, rng.randint(lo, hi)))
        offs.append(len(out))
        out += h + pay
    return out, offs


# ---- 1. lengths parse, CRC wrong ---------------------------------------------------------------------------------
@pytest.mark.parametrize("comp", [0, 2], ids=["none", "snappy"])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_lengths_parse_crc_wrong(where, comp, monkeypatch):
    """A header whose magic, nil byte, sizes and CRC varint all parse (the next header's load goes out on them) and
    whose CRC-32C is wrong, as the first, a middle and the last record of a lane chunk: the oracle's header-CRC
    error with its expected and actual values, every record before it delivered and none after."""
    chunk = 4096
    img, offs = _records_file(4, comp, 400, seed=11 + comp, lo=40, hi=700)
    k = 5  # a chunk in the middle of the file
    inside = [i for i, p in enumerate(offs) if 8 + k * chunk <= p < 8 + (k + 1) * chunk]
    assert len(inside) >= 3
    bad = {"first": inside[0], "middle": inside[len(inside) // 2], "last": inside[-1]}[where]
    p = offs[bad]
    q = p + 4  # u, c, then the CRC varint: flip a payload bit of its first byte (its length stays)
    for _ in range(2):
        while img[q] & 0x80:
            q += 1
        q += 1
    img[q] ^= 0x01
    g, o = _check(_lane_decoder(monkeypatch, chunk), f"crc@{where}", img)
    assert o["status"] == STATUS["HEADER_CRC"] and g["n_records"] == bad and g["status_offset"] == p


# ---- 2. lengths that lie ---------------------------------------------------------------------------------------
def _lying_header(version, comp, plen, nbytes=None):
    """A header of this version whose payload length field (c with a codec, else u) says plen; v4: under a valid CRC."""
    enc = (lambda v: padded_uvarint(v, nbytes)) if nbytes else uvarint
    other = uvarint(7)
    ub, cb = (other, enc(plen)) if comp else (enc(plen), uvarint(0))
    if version == 4:
        return header_v4(0, 0, u_bytes=ub, c_bytes=cb)
    if version == 3:
        return MAGIC + b"\x00" + ub + cb
    return MAGIC + ub + cb


@pytest.mark.parametrize("version,comp", [(4, 0), (4, 2), (3, 0), (2, 0)], ids=["v4-none", "v4-snappy", "v3", "v2"])
def test_lengths_that_lie(version, comp, monkeypatch):
    """A header in the middle of a lane chunk, reached by a hop, whose unverified length would be used as an address:
    the next record at the file's end, 1, 31, 32 and 33 bytes before it (around the walk's 32-byte window), far past
    the end, and a 10-byte varint whose sum with the offset wraps 2^64. v2 and v3 headers have no CRC to stop them."""
    dec = _lane_decoder(monkeypatch, 1024)
    body, _ = _records_file(version, comp, 60, seed=21)
    tail = _payload(random.Random(22), 300)
    cases = [(f"len-{d}", len(tail) - d, None) for d in (0, 1, 31, 32, 33)]
    cases += [("far", 1 << 40, None), ("wrap", (1 << 64) - 40, 10), ("wrap-max", (1 << 64) - 1, 10)]
    for name, plen, nbytes in cases:
        h = _lying_header(version, comp, plen, nbytes)
        img = bytes(body) + h + tail
        if name.startswith("len-"):  # the claimed next record start, against the file's length
            assert len(body) + len(h) + plen == len(img) - int(name[4:])
        _check(dec, f"v{version}/{comp} {name}", img)
        # and with a true record behind the liar's claimed end, where there is room for one
        if name in ("len-32", "len-33"):
            h2, pay2 = _record(version, 0, b"0123456789")
            if comp == 0:
                cut = len(img) - int(name[4:])
                _check(dec, f"v{version} {name} then a header", img[:cut] + h2 + pay2)


# ---- 3. truncations --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("comp", [0, 2], ids=["none", "snappy"])
def test_truncations_around_the_window(comp, monkeypatch):
    """The file cut 0 .. 40 bytes behind its last header's start: the cuts fall inside the header, at its end, and
    on both sides of the 32 bytes the walk loads for it."""
    dec = _lane_decoder(monkeypatch, 512)
    img, offs = _records_file(4, comp, 80, seed=31, lo=60, hi=400)
    for cut in range(41):
        _check(dec, f"cut+{cut}", img[: offs[-1] + cut])


# ---- 4. entry hand-over ----------------------------------------------------------------------------------------
def _file_with_headers_at(chunk, line_offsets, seed, fakes=()):
    """A v4 uncompressed file where chunk k = 1, 2, .. holds no header before the one at line offset line_offsets[k - 1]
    of the chunk's second 128-byte line ("last": at the chunk's last byte): a record starting before the chunk ends
    exactly there. fakes: (k, line, offset) positions of `91 8d 4c` written into that record's payload."""
    rng = random.Random(seed)
    out = bytearray(file_header(4, 0))
    targets = []

    def add(n):
        nonlocal out
        out += header_v4(n, 0) + _payload(rng, n)

    for k, off in enumerate(line_offsets, start=1):
        cs, ce = 8 + k * chunk, 8 + (k + 1) * chunk
        t = ce - 1 if off == "last" else (cs & ~127) + 128 + off
        assert cs <= t < ce
        while cs - len(out) > 110:  # records up to 60 .. 110 bytes before the chunk
            add(min(rng.randint(40, 300), cs - len(out) - 69))
        # the record [len(out), t): starts before the chunk, ends at the target. Its header's length varies with the
        # payload's length and the CRC's value: where no payload length fits, a 40-byte record first moves its start.
        while True:
            total = t - len(out)
            n = next((n for n in range(total - 14, total - 5) if len(header_v4(n, 0)) + n == total), None)
            if n is not None:
                break
            add(40)
        assert len(out) < cs and 40 <= n <= 1100, (k, len(out), cs, n)
        out += header_v4(n, 0)
        out += _payload(rng, n)
        assert len(out) == t
        targets.append(t)
    for _ in range(6):
        add(rng.randint(40, 300))
    for k, line, off in fakes:
        q = ((8 + k * chunk) & ~127) + 128 * line + off
        assert q + 3 <= targets[k - 1] and q >= 8 + k * chunk
        out[q:q + 3] = MAGIC
    return out, targets


@pytest.mark.parametrize("chunk", [512, 992])
def test_entry_header_at_line_edges(chunk, monkeypatch):
    """A chunk's first header at line offsets 0, 95, 96, 97 (at 96 its 32 bytes end with the line), 125 .. 127 (the
    magic itself crosses into the next line the search holds) and at the chunk's last byte."""
    offs = [0, 95, 96, 97, 125, 126, 127, "last"]
    img, targets = _file_with_headers_at(chunk, offs, seed=41)
    g, o = _check(_lane_decoder(monkeypatch, chunk), f"entry@{chunk}", img)
    assert o["status"] == STATUS["EOF"] and set(targets) <= set(int(x) for x in o["rec_off"])
    assert g["n_repairs"] == 0


def test_entry_false_magic_before_the_header(monkeypatch):
    """`91 8d 4c` in a payload ahead of the chunk's true header: in the same line (chunk 1), and with the true header
    in the next line (chunk 2: the false one at the line's end, its 32 bytes reaching over the header)."""
    chunk = 512
    img, targets = _file_with_headers_at(chunk, [100, 10, 64], seed=42, fakes=[(1, 1, 40), (2, 0, 120), (3, 1, 61)])
    g, o = _check(_lane_decoder(monkeypatch, chunk), "false magic", img)
    assert o["status"] == STATUS["EOF"] and set(targets) <= set(int(x) for x in o["rec_off"])


def test_chunks_without_a_header(monkeypatch):
    """Records that span whole lane chunks: those chunks have no entry."""
    rng = random.Random(43)
    recs = [_payload(rng, rng.choice([40, 90, 700, 1100])) for _ in range(200)]
    img = file_header(4, 0) + b"".join(header_v4(len(r), 0) + r for r in recs)
    for chunk in (64, 256):
        _check(_lane_decoder(monkeypatch, chunk), f"spanning@{chunk}", img)


def test_embedded_false_headers_still_repair(monkeypatch):
    """The corpus' CRC-valid false headers (recordio files as payloads): a lane's entry is handed to the walk framed,
    breaks at the stitch, and the scan repairs it."""
    g, _ = _check(_lane_decoder(monkeypatch, 4096), "mixed_c0_embedded", dict(corpus.cases())["mixed_c0_embedded"])
    assert g["n_repairs"] > 0


# ---- 5. dispatch -----------------------------------------------------------------------------------------------
def _record_set():
    recs = corpus.mixed_records(600, seed=51, max_len=1100)
    recs[3], recs[4], recs[5] = None, b"", None  # nil and empty records next to each other
    return recs


@pytest.mark.parametrize("version,comp", [(1, 0), (1, 2), (2, 0), (2, 2), (3, 0), (3, 2), (4, 0), (4, 2), (4, 1), (4, 3)],
                         ids=["v1-none", "v1-snappy", "v2-none", "v2-snappy", "v3-none", "v3-snappy", "v4-none",
                              "v4-snappy", "v4-gzip", "v4-lzw"])
def test_every_version_and_codec(version, comp, monkeypatch):
    """One record set (nil and empty records among it) in every layout: v4 none / snappy through their own
    instantiations, everything else through the generic code."""
    from recordio import encode_file

    recs = _record_set()
    if version == 4:
        img = encode_file(recs, comp)
    elif version == 3:
        img = corpus.v3_file(recs, comp)
    else:
        img = corpus.legacy_file(recs, comp, version)
    assert struct.unpack_from("<II", img, 0) == (version, comp)
    g, o = _check(_lane_decoder(monkeypatch, 1024), f"v{version}/{comp}", img)
    assert o["status"] == STATUS["EOF"] and g["n_records"] == len(recs)


@pytest.mark.parametrize("comp", [0, 2], ids=["none", "snappy"])
def test_header_lengths_19_20_21(comp, monkeypatch):
    """Non-canonical varints that make the v4 header 19, 20 and 21 bytes long: with snappy the preamble is read from
    the walk's 32 bytes only while the header is at most 20."""
    rng = random.Random(52)
    out = bytearray(file_header(4, comp))
    for i in range(300):
        data = _payload(rng, rng.randint(40, 600))
        pay = corpus.snappy_encode(data) if comp else data
        nu, nc = [(5, 5), (5, 6), (6, 6), (0, 0)][i % 4]  # + magic 3, nil 1, CRC 5
        if nu:
            pre = MAGIC + b"\x00" + padded_uvarint(len(data), nu) + padded_uvarint(len(pay) if comp else 0, nc)
            h = pre + padded_uvarint(crc32c(pre), 5)
            assert len(h) == 9 + nu + nc  # 19, 20, 21
        else:
            h = header_v4(len(data), len(pay) if comp else 0)
        out += h + pay
    g, o = _check(_lane_decoder(monkeypatch, 512), f"hl 19..21 /{comp}", out)
    assert o["status"] == STATUS["EOF"] and g["n_records"] == 300


# ---- 6. geometry -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_chunks", [1, 63, 64, 65, 257])
def test_lane_chunk_counts(n_chunks, monkeypatch):
    """Files of 1, 63, 64, 65 and 257 lane chunks: a partial wave, exactly one, one lane more, several workgroups."""
    chunk = 256
    rng = random.Random(61)
    out = bytearray(file_header(4, 2))
    while len(out) - 8 <= (n_chunks - 1) * chunk:  # a record is shorter than a chunk: the last one ends in the last chunk
        h, pay = _record(4, 2, _payload(rng, rng.randint(40, 200)))
        assert len(h) + len(pay) < chunk
        out += h + pay
    assert (len(out) - 8 + chunk - 1) // chunk == n_chunks
    g, o = _check(_lane_decoder(monkeypatch, chunk), f"{n_chunks} chunks", out)
    assert g["n_chunks"] == n_chunks and o["status"] == STATUS["EOF"]
