"""The lane-stream tests' inputs, checked on the host (no GPU).

tests/test_gpu_snappy_lane_stream.py decodes the files of snappy_streams.CASES on the device and
compares them with the oracle. What that proves depends on what the files hold and where the launch
puts it: this module checks both, the record forms against the oracle's golang/snappy restatement
(orc_snappy_decode), and every file against tests/lane_split.py, the mirror of the two
record-to-lane splits.
"""
import random

import numpy as np
import pytest

import corpus
import oracle_py as orc
import snappy_streams as S
from lane_split import CHUNKS_PER_WAVE, WAVES, batch_split, pipe_split
from recordio import _lib as L

BIG = 20_000  # files of fewer records (the 65-record files of "need") cannot hold every pair of forms


@pytest.mark.parametrize("name", S.ALL)
def test_form_verdict_is_the_oracles(name):
    """Every form's oracle verdict equals its `valid` flag, as a block (Decode) and as the one
    record of a file (ReadNext); a valid form's bytes are the builder's own."""
    for seed in range(6):
        payload, decoded, valid = S.FORMS[name](random.Random(seed))
        assert valid == (name in S.VALID)
        if payload is not None:
            st, out = orc.snappy_decode(payload)
            assert (st == 0) == valid, (name, seed, st)
            if valid:
                assert out == decoded
            else:
                assert st == L.RIO_ERR_DECOMPRESS and decoded is None
        o = orc.file_reader_decode(corpus.file_header(4, 2) + S.frame(payload))
        assert o["status"] == L.RIO_EOF and o["n_records"] == 1
        rec = o["records"][0]
        if not valid:
            assert isinstance(rec, orc.BadRecord) and o["n_bad"] == 1
        elif payload is None:
            assert rec is None
        else:
            assert rec == decoded and o["n_bad"] == 0


@pytest.mark.parametrize("tag", [62, 63])
@pytest.mark.parametrize("n", [1, 5, 60, 61, 256, 257, 65536, 70001])
def test_long_literal_length_forms(tag, n):
    body = bytes(i * 7 & 0xFF for i in range(n))
    st = S.Stream()
    st.literal(body, tag)
    assert len(st.els) == 1 + (tag - 59) + n
    assert orc.snappy_decode(st.payload()) == (0, body)


def test_copy4_decodes():
    st = S.Stream()
    st.literal(b"abcd")
    st.copy4(2, 7)
    assert st.els[5] & 3 == 3 and len(st.els) == 10
    assert orc.snappy_decode(st.payload()) == (0, b"abcdcdcdcdc")


def test_edge_matrix_is_full_and_valid():
    sts = S.edge_matrix()
    assert len(sts) == 16 * 4 * len(S.EDGE_LENS)
    o = orc.file_reader_decode(S.file_of(sts))
    assert o["status"] == L.RIO_EOF and o["n_bad"] == 0
    assert o["records"] == [bytes(st.out) for st in sts]


@pytest.fixture(scope="module", params=list(S.CASES))
def case(request):
    """One case of the table: its files, the mirror's split of them, and the oracle's decode."""
    name = request.param
    tiles = S.case_tiles(name)
    if name.startswith("single"):
        per, lanes = pipe_split(tiles[0].n)
        split = [lanes]
    else:
        per, split = batch_split([t.n for t in tiles])
    split = [np.array(lanes, dtype=np.int64).reshape(-1, 2) for lanes in split]
    oracles = [orc.file_reader_decode_arrays(t.image) for t in tiles]
    return name, per, tiles, split, oracles


def lane_view(t, lanes):
    """Per record: its lane, and whether it is the first / a middle / the last of a lane that holds
    more than one record. Asserts that the lanes' ranges are the file's records, in order, once."""
    r0, r1 = lanes[:, 0], lanes[:, 1]
    size = r1 - r0
    live = size > 0
    assert r0[live][0] == 0 and r1[live][-1] == t.n and np.array_equal(r0[live][1:], r1[live][:-1])
    lane = np.repeat(np.arange(len(lanes)), size)
    i = np.arange(t.n)
    several = size[lane] > 1
    first, last = several & (i == r0[lane]), several & (i == r1[lane] - 1)
    return lane, size, first, several & ~first & ~last, last


def test_case_reaches_the_records_per_lane_it_names(case):
    name, per, tiles, split, _ = case
    assert per == S.CASES[name][0]
    counts = [t.n for t in tiles]
    if name.startswith("single"):
        assert counts[0] >= 2 * CHUNKS_PER_WAVE * 64 * WAVES
    elif name == "need":  # the first guess is 1 record per lane, and it needs more waves than there are
        assert sum(counts) <= 64 * WAVES and sum((n + 63) // 64 for n in counts) > WAVES
    else:  # "just over" (per - 1) records for each lane of the grid
        assert 0 < sum(counts) - (per - 1) * 64 * WAVES < 1000
        assert any(n % (64 * per) for n in counts)
    # one launch group (kMaxBatch = 16), with room for the file that takes no part where the GPU test adds one
    assert len(tiles) <= (16 if name == "need" else 15)


def test_every_pair_position_and_offset_inside_the_lanes(case):
    name, per, tiles, split, oracles = case
    short = False
    for k, (t, lanes, o) in enumerate(zip(tiles, split, oracles)):
        what = f"{name}[{k}]"
        lane, size, first, middle, last = lane_view(t, lanes)
        short = short or bool(((size > 0) & (size < per)).any())
        # the wave that starts at the arena's first bytes (kLow) is the file's first, it alone, and holds a far copy
        w0 = lanes[0:64]
        assert t.far[w0[0, 0]:w0[-1, 1]].any(), what
        heads = lanes[64::64, 0]
        assert (o["out_off"][heads[heads < t.n]] >= 3).all(), what
        if t.n < BIG:
            continue
        nf = len(t.names)
        seq = t.seq.astype(np.int64)
        same = lane[:-1] == lane[1:]
        assert np.unique(seq[:-1][same] * nf + seq[1:][same]).size == nf * nf, what
        assert np.unique(seq[first]).size == nf and np.unique(seq[last]).size == nf, what
        if per >= 3:
            assert np.unique(seq[middle]).size == nf, what
        assert np.unique(seq * 16 + o["rec_off"] % 16).size == nf * 16, what
    assert short, name


def test_failing_lanes_listed_or_overflowing(case):
    name, per, tiles, split, _ = case
    for k, (t, lanes) in enumerate(zip(tiles, split)):
        lane = lane_view(t, lanes)[0]
        failing = np.unique(lane[~t.valid]).size
        if name in ("listed", "single_rpc2"):
            assert 1 <= failing <= S.FAIL_LANES, (k, failing)
        elif name in ("overflow", "single_rpc2_overflow"):
            assert failing > S.FAIL_LANES, (k, failing)
        else:
            assert failing == 0


def test_oracle_flags_exactly_the_invalid_records(case):
    """The device comparison leaves the bytes of flagged records out; so the flagged records must
    be the invalid forms and nothing else, and few."""
    name, per, tiles, split, oracles = case
    for k, (t, o) in enumerate(zip(tiles, oracles)):
        assert o["status"] == L.RIO_EOF and o["n_records"] == t.n, (name, k)
        assert o["n_bad"] == t.n_invalid and t.n_invalid * 10 < t.n, (name, k, o["n_bad"], t.n_invalid)
        assert np.array_equal((o["flags"] & L.RIO_FLAG_CORRUPT) != 0, ~t.valid), (name, k)
        assert np.array_equal((o["flags"] & L.RIO_FLAG_NIL) != 0, t.seq == t.names.index("nil")), (name, k)
