"""The hand-built DEFLATE families (tests/deflate_cases.py) on the CPU: the builder's expansion, the
tracer (Go's rules, its own inflate), the oracle (zlib's inflate under Go's gzip framing) and, for
valid streams, zlib itself agree on every record, and every family produces the decoder branches it
declares (which keeps tests/test_gpu_gzip_edges.py meaningful)."""
import zlib

import pytest

import corpus
import deflate_cases as D
import oracle_py as orc

FAMILIES = [f.__name__ for f in D.VALID_FAMILIES + D.REFUSED_FAMILIES]


def family(name):
    return D.cached(next(f for f in D.VALID_FAMILIES + D.REFUSED_FAMILIES if f.__name__ == name))


def zlib_members(payload):
    """The payload's members through zlib's raw inflate (10-byte headers, 8-byte trailers skipped)."""
    out, p = b"", payload
    while p:
        z = zlib.decompressobj(-15)
        out += z.decompress(p[10:])
        assert z.eof
        p = z.unused_data[8:]
    return out


def oracle_record(case):
    o = orc.file_reader_decode(corpus.gz_file([case.item]))
    assert o["n_records"] == 1
    return o["records"][0]


@pytest.mark.parametrize("name", FAMILIES)
def test_builder_tracer_oracle_and_zlib_agree(name):
    for c in family(name).cases:
        res, _ = D.traced(c)
        assert res == c.expect, (name, c.name)
        r = oracle_record(c)
        if c.valid:
            assert r == c.expect, (name, c.name)
            assert zlib_members(c.payload) == c.expect, (name, c.name)
            assert c.u == len(c.expect)
        else:
            assert r == orc.BadRecord("corrupt"), (name, c.name, r)


@pytest.mark.parametrize("name", FAMILIES)
def test_family_produces_the_branches_it_declares(name):
    f = family(name)
    union = set()
    for c in f.cases:
        lab = D.traced(c)[1]
        union |= lab
        missing = f.per_case.get(c.name, set()) - lab
        assert not missing, (name, c.name, sorted(missing))
    assert not f.labels - union, (name, sorted(f.labels - union))
    assert not set(f.per_case) - {c.name for c in f.cases}


def test_refused_records_are_refused_and_valid_ones_valid():
    for fn in D.VALID_FAMILIES:
        f = D.cached(fn)
        bad = [c.name for c in f.cases if not c.valid]
        assert bad == [c.name for c in f.cases if c.name.startswith("isize_")], (f.name, bad)  # ISIZE lies only
    assert not any(c.valid for c in D.cached(D.refused_family).cases)
    cut = D.cached(D.cut_body_family).cases
    assert [c.name for c in cut if c.valid] == ["uncut"] and len(cut) > 130
    for c in cut[:-1]:  # the last four payload bytes stay the true ISIZE: the framing's size is sane
        assert c.payload[-4:] == cut[-1].payload[-4:] and c.u == len(cut[-1].expect)


def test_size_classes_of_the_match_family():
    f = D.cached(D.match_family)
    for c in f.cases:
        n = len(c.expect)
        if c.name.startswith("large_d"):
            assert n > 2048, c.name
        elif c.name.startswith("cls0_"):
            assert n <= 1024, c.name
        elif c.name.startswith("cls1_"):
            assert 1024 < n <= 2048, c.name
    for cls in (0, 1):
        got = set()
        for c in f.cases:
            if c.name.startswith(f"cls{cls}_"):
                got |= {x for x in D.traced(c)[1] if x.startswith("m")}
        want = {f"m{ln}@{d}" for ln in D.SMALL_LENS for d in range(1, 65)}
        assert not want - got, (cls, sorted(want - got)[:10])


def test_wide_token_payload_sizes():
    by = {c.name: c for c in D.cached(D.wide_token_family).cases}
    assert len(by["wide_8k"].payload) >= 8192 and len(by["wide_64k"].payload) >= 65536
    assert len(by["wide_tiny"].expect) <= 1024 and len(by["wide_tiny_literals"].expect) <= 1024
    assert len(by["wide_tiny_literals"].payload) > 4 * 256


def test_neighbours_mix_every_kind_in_every_position():
    items = D.neighbour_family()
    assert len(items) % 16 == 0 and len(items) >= 400
    kind = lambda c: "nil" if c is None else c.name.split("_", 1)[1]  # noqa: E731
    at = {k: set() for k in D.NEIGHBOUR_KINDS}
    beside = {k: set() for k in D.NEIGHBOUR_KINDS}
    for g in range(0, len(items), 4):
        four = [kind(c) for c in items[g:g + 4]]
        assert len(set(four)) == 4, four
        for j, k in enumerate(four):
            at[k].add(j)
            beside[k] |= set(four) - {k}
    for k in D.NEIGHBOUR_KINDS:
        assert at[k] == {0, 1, 2, 3}, (k, at[k])
        assert beside[k] == set(D.NEIGHBOUR_KINDS) - {k}, (k, beside[k])
    # the oracle on every record; the tracer on all but the 3000-block ones, of which it walks three
    image = corpus.gz_file([None if c is None else c.item for c in items])
    o = orc.file_reader_decode(image)
    assert o["n_records"] == len(items)
    slow = 0
    for c, r in zip(items, o["records"]):
        if c is None:
            assert r is None
            continue
        assert (r == c.expect) if c.valid else (r == orc.BadRecord("corrupt")), c.name
        assert len(c.expect if c.valid else b"") <= 1024, c.name
        if c.name.endswith("empty3000"):
            slow += 1
            if slow > 3:
                continue
        assert D.trace(c.payload)[0] == c.expect, c.name


def test_shuffled_file_holds_every_family():
    img, cases = D.shuffled_all()
    names = {c.name for c in cases if c is not None}
    for f in D.families():
        for c in f.cases:
            assert c.name in names or c.name.startswith("large_d"), c.name
    assert sum(1 for c in cases if c is not None and c.name.startswith("large_d")) == 40
    o = orc.file_reader_decode(img)
    assert o["n_records"] == len(cases)
    for c, r in zip(cases, o["records"]):
        if c is None:
            assert r is None
        elif c.valid:
            assert r == c.expect, c.name
        else:
            assert r == orc.BadRecord("corrupt"), c.name


def test_redo_file_is_what_it_claims():
    img, recs, redo = D.redo_file()
    assert len(img) > 1536 * 256 and redo[0] == 49 and len(redo) == 50
    o = orc.file_reader_decode(img)
    assert o["records"] == recs and o["n_bad"] == 0
    for i in (48, 49, 50, 2499):
        assert D.trace(corpus.gzip_members(recs[i], [len(recs[i]) // 3]))[1] >= {"members=2"}


def test_tracer_on_zlib_output():
    """The tracer is an inflate in its own right: zlib's streams at every level and strategy."""
    for r in corpus.text_records(12, 3, 1, 3000):
        for lvl, st in ((0, 0), (1, 0), (9, 0), (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE)):
            assert D.trace(corpus.gzip_member(r, lvl, st))[0] == r
        assert D.trace(corpus.gzip_members(r, [len(r) // 2]))[0] == r
        p = corpus.gzip_member(r)
        assert D.trace(p[:-8] + bytes([p[-8] ^ 1]) + p[-7:])[0] == D.CORRUPT
        assert D.trace(p[:len(p) // 2])[0] == D.CORRUPT
