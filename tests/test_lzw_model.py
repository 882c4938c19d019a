"""Go's compress/lzw reader restated twice (tests/lzw_model.py in Python, oracle/rio_oracle.c in C): the
two agree on the crafted streams (full table without a clear, code == hi at the width steps, KwKwK
chains, 16-bit position edges) and on every payload of corpus.lzw_cases(). The streams are what they
claim (tests/test_gpu_lzw_edges.py runs them on the device)."""
import struct

import pytest

import corpus
import lzw_model as M
import oracle_py as orc

ITEMS = M.case_items()


def oracle(payload):
    st, b = orc.lzw_decode(payload)
    return b if st == 0 else M.CORRUPT


def codes_of(payload):
    """The code list of a payload up to its eof / end, with each code's epoch index."""
    bits = nb = k = ip = 0
    out = []
    while True:
        w = M.width_of(k)
        while nb < w:
            if ip >= len(payload):
                return out
            bits |= payload[ip] << nb
            ip += 1
            nb += 8
        c = bits & ((1 << w) - 1)
        bits >>= w
        nb -= w
        out.append((k, c))
        if c == M.EOF:
            return out
        k = 0 if c == M.CLEAR else k + 1


@pytest.mark.parametrize("name,item,want", ITEMS, ids=[i[0] for i in ITEMS])
def test_model_equals_oracle(name, item, want):
    assert oracle(item[1]) == want
    assert (want is M.CORRUPT) == name.startswith("bad_")


def payloads(img):
    """(payload or None for nil) of every record of an lzw image (v1 .. v4 headers)."""
    ver = struct.unpack_from("<I", img, 0)[0]
    p, out = 8, []

    def uv(i):
        v = s = 0
        while True:
            c = img[i]
            i += 1
            v |= (c & 0x7F) << s
            s += 7
            if c < 0x80:
                return v, i
    while p < len(img):
        nil = False
        if ver == 1:
            _, _, c = struct.unpack_from("<IQQ", img, p)
            q = p + 20
        else:
            q = p + 3
            if ver >= 3:
                nil = img[q] == 1
                q += 1
            _, q = uv(q)
            c, q = uv(q)
            if ver == 4:
                _, q = uv(q)
        out.append(None if nil else img[q:q + c])
        p = q + (0 if nil else c)
    return out


@pytest.mark.parametrize("name,image", corpus.lzw_cases(), ids=[c[0] for c in corpus.lzw_cases()])
def test_model_equals_oracle_on_the_corpus(name, image):
    o = orc.file_reader_decode(image)
    pays = payloads(image)
    assert len(pays) == o["n_records"], name
    for p, r in zip(pays, o["records"]):
        if p is None:
            assert r is None
        elif len(p) == 0:
            assert isinstance(r, orc.BadRecord)  # (lzw: io.ErrUnexpectedEOF; the model says CORRUPT too)
            assert M.decode(p) == M.CORRUPT
        else:
            want = M.decode(p)
            assert (r == want) if want is not M.CORRUPT else (r == orc.BadRecord("corrupt")), name


def test_files_agree_with_the_oracle():
    assert tuple(f[0] for f in M.files()) == M.FILE_NAMES
    for name, img, exp in M.files():
        o = orc.file_reader_decode(img)
        assert o["n_records"] == len(exp), name
        for r, want in zip(o["records"], exp):
            assert (r == want) if want is not M.CORRUPT else (r == orc.BadRecord("corrupt")), name


def test_streams_are_what_they_claim():
    by = {n: it[1] for n, it, _ in ITEMS}
    res = {n: r for n, _, r in ITEMS}
    # full table: no clear between epoch index 0 and the codes past 3838; 4095 at 3838 and at 3839
    for n in ("full_4094_then_4095", "full_kwkwk_at_3838", "full_then_6000", "full_then_clear"):
        cs = codes_of(by[n])
        assert max(k for k, _ in cs) >= 3845, n
    cs = dict(codes_of(by["full_kwkwk_at_3838"]))
    assert cs[3837] < 256 and cs[3838] == cs[3839] == cs[3840] == 4095
    cs = dict(codes_of(by["full_4094_then_4095"]))
    assert (cs[3838], cs[3839], cs[3840]) == (4094, 4095, 4095)
    assert max(k for k, _ in codes_of(by["full_then_6000"])) > 9800
    cs = codes_of(by["full_then_clear"])
    assert [k for k, c in cs if c == M.CLEAR][1:] == [3900, 700]
    cs = codes_of(by["full_after_63"])
    assert cs[64] == (63, M.CLEAR) and cs[64 + 3839] == (3838, 4095)
    # code == hi and hi + 1 where the width changes
    for k in (255, 767, 1791):
        assert dict(codes_of(by[f"kwkwk_at_{k}"]))[k] == 257 + k
        assert dict(codes_of(by[f"bad_hi_plus_1_at_{k}"]))[k] == 258 + k
        assert M.width_of(k) == M.width_of(k - 1) + 1
    # chains: at least 64 consecutive codes that are the entry being defined
    for n in (64, 65, 130, 200):
        cs = codes_of(by[f"kwkwk_chain_{n}"])
        run = [c == 257 + k for k, c in cs]
        assert sum(run) >= n and all(run[2:2 + n])
    # class edges: same payload size, 65535 bytes (small class: slen <= 1152, < 65536 decoded) and 65536
    assert len(by["decodes_to_65535"]) == len(by["decodes_to_65536"]) <= 1152
    assert (len(res["decodes_to_65535"]), len(res["decodes_to_65536"])) == (65535, 65536)
    for size in (1151, 1152, 1153):
        assert len(by[f"payload_{size}"]) == size
        assert len(codes_of(by[f"payload_{size}"])) > 850  # the codes fill the payload


def test_redo_file_is_what_it_claims():
    img, recs, redo = M.redo_file()
    assert len(img) > 1536 * 256 and redo[0] == 49 and len(redo) == 50
    o = orc.file_reader_decode(img)
    assert o["records"] == recs and o["n_bad"] == 0
    us = [len(r) for r in recs]
    hdr = [u for u, _ in M_items(img)]
    assert [i for i, (a, b) in enumerate(zip(us, hdr)) if a != b] == redo


def M_items(img):
    """(u, c) of every v4 record header of an image."""
    p, out = 8, []

    def uv(i):
        v = s = 0
        while True:
            c = img[i]
            i += 1
            v |= (c & 0x7F) << s
            s += 7
            if c < 0x80:
                return v, i
    while p < len(img):
        u, q = uv(p + 4)
        c, q = uv(q)
        _, q = uv(q)
        out.append((u, c))
        p = q + c
    return out
