"""The encoder edge families (tests/encode_cases.py) on the CPU: the oracle's streams parse under the
format's rules and carry every class a family declares (which keeps tests/test_gpu_encode_edges.py
meaningful), decode back to the input, and the host writer (rio_writer.cpp) equals the oracle."""
import numpy as np
import pytest

import encode_cases as E
import oracle_py as orc
from recordio import encode_file

FAMILY_NAMES = [f.name for f in E.cached_families()]


def family(name):
    return next(f for f in E.cached_families() if f.name == name)


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_family_parses_and_covers_its_classes(name):
    f = family(name)
    union = set()
    for i, r in enumerate(f.records):
        lab = E.classes(E.oracle_snappy(r or b""))
        union |= lab
        missing = f.per_record.get(i, set()) - lab
        assert not missing, (name, i, sorted(missing))
    assert not f.classes - union, (name, sorted(f.classes - union))


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_family_round_trips_through_the_decoder(name):
    for i, r in enumerate(family(name).records):
        st, back = orc.snappy_decode(E.oracle_snappy(r or b""))
        assert st == 0 and back == (r or b""), (name, i)


@pytest.mark.parametrize("comp", [0, 2])
@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_host_writer_equals_oracle(name, comp):
    recs = family(name).records
    want, offs = orc.encode_file(recs, comp)
    assert encode_file(recs, comp) == want
    if comp == 2:  # the file's payloads are the streams the class test looked at
        for r, (nil, u, c, pay) in zip(recs, E.payloads(want, offs)):
            assert (nil, u, c) == (r is None, len(r or b""), len(E.oracle_snappy(r or b"")))
            assert pay == (b"" if r is None else E.oracle_snappy(r))


@pytest.mark.parametrize("comp", [0, 2])
def test_nil_record_with_a_span_is_skipped(comp):
    (blob, off, flags), same_as = E.nil_span_batch()
    img, offs = E.oracle_arrays(blob, off, flags, comp)
    want, want_offs = orc.encode_file(same_as, comp)
    assert img.tobytes() == want and offs.tolist() == want_offs
    assert want == encode_file(same_as, comp)
    p = E.payloads(want, want_offs)
    assert (p[0][:2], p[2][:2]) == ((0, 200), (0, 1500))
    assert p[1] == (1, 0, 1 if comp == 2 else 0, b"")  # c = len(snappy.Encode(nil)) = 1, no payload


def test_shuffled_batch_is_the_families():
    items = E.shuffled_all()
    assert len(items) == sum(len(f.records) for f in E.cached_families())
    assert sorted((n, i) for n, i, _ in items) == sorted((f.name, i) for f in E.cached_families()
                                                         for i in range(len(f.records)))
    assert [x[:2] for x in items] != sorted(x[:2] for x in items)


def test_launch_shapes_are_what_they_claim():
    blob, off, flags = E.launch_global_reuse()
    lens = np.diff(off).astype(np.int64)
    assert len(lens) == 8192 + 64 + 1 and int(lens.min()) >= 1025
    big = np.nonzero(lens > 1100)[0].tolist()
    assert lens[big].tolist() == [70000] * 3 and big[0] < 8192 < big[1] and big[1] - big[0] == 8192
    blob, off, flags = E.launch_lds_second_pass()
    lens = np.diff(off).astype(np.int64)
    assert len(lens) == 262144 + 16 + 1 and 17 == lens.min() and lens.max() == 40
    blob, off, flags = E.launch_million_tiny()
    lens = np.diff(off).astype(np.int64)
    assert len(lens) == 1048576 + 300 and lens.min() == 0 and lens.max() == 3
    assert 0 < int(flags.sum()) < len(lens) // 8 and int((flags.astype(bool) & (lens > 0)).sum()) > 0


# ---- the parser itself: it must refuse what golang/snappy never emits ---------------------------
def lit(n):
    return bytes([(n - 1) << 2]) + bytes(range(n))


@pytest.mark.parametrize("stream,why", [
    (bytes([8]) + lit(4) + bytes([3 << 2 | 3, 4, 0, 0, 0]), "4-byte offset"),
    (bytes([4]) + bytes([62 << 2, 3, 0, 0]) + bytes(4), "3-byte literal length"),
    (bytes([8]) + lit(4) + bytes([0 << 2 | 1, 5]), "offset beyond the output"),
    (bytes([8]) + lit(4) + bytes([0 << 2 | 1, 0]), "offset 0"),
    (bytes([8]) + lit(4) + bytes([3 << 2 | 2, 4, 0]), "tag-10 copy of 4 at a near offset, no chain"),
    (bytes([9]) + lit(4) + bytes([0 << 2 | 1, 4]), "lengths do not sum to the preamble"),
    (bytes([8]) + lit(4) + bytes([0 << 2 | 1, 4, 0]), "trailing byte"),
])
def test_parser_refuses(stream, why):
    with pytest.raises((AssertionError, IndexError)):
        E.elements(stream)


def test_parser_accepts_chain_ends_and_far_short_copies():
    # literal 4, then a 69-byte match at offset 4 the way emitCopy splits it: 64 + 5 as tag 10
    s = bytes([73]) + lit(4) + bytes([63 << 2 | 2, 4, 0]) + bytes([4 << 2 | 2, 4, 0])
    assert [e[:3] for e in E.elements(s)] == [("lit1", 4, 0), ("c2", 64, 4), ("c2", 5, 4)]
    assert {"copy=69", "split=64+5", "overlap", "tail[0]=0"} <= E.classes(s)
    with pytest.raises(AssertionError):  # emitCopy never leaves 64 + 6 as 60 + 10
        E.classes(bytes([74]) + lit(4) + bytes([59 << 2 | 2, 4, 0]) + bytes([9 << 2 | 2, 4, 0]))
    assert [E.split_copy(n) for n in (64, 65, 67, 68, 124, 132)] == [[64], [60, 5], [60, 7], [64, 4], [64, 60],
                                                                     [64, 64, 4]]
