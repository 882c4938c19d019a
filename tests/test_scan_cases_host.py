"""The files of tests/scan_cases.py against the oracle, on the CPU: what their ledgers claim is what FileReader
reads, the ledgers list every 91 8d 4c of their images with the right claim about each, every case has the chunk,
block and tile counts it is named for and its event where its name says, and the sequential model gives the
repair count each break was engineered for. tests/test_gpu_chunk_scan.py then holds the device to the same list:
this module is where the list itself is held to the reference."""
import numpy as np
import pytest

import oracle_py as orc
import scan_cases as SC
from conftest import STATUS

GROUP_IDS = list(SC.GROUPS)


def check_case(case: SC.Case):
    img, led, m = SC.built(case.id)
    what = case.id
    # the ledger's chain is the oracle's
    o = orc.file_reader_decode_arrays(img)
    assert o["status"] == STATUS[led.status], (what, o["status"], led.status)
    assert o["status_offset"] == led.status_offset, (what, o["status_offset"], led.status_offset)
    if led.status == "HEADER_CRC":
        assert (o["detail0"], o["detail1"]) == led.detail, what
    np.testing.assert_array_equal(o["rec_off"], led.rec_off, err_msg=what)
    np.testing.assert_array_equal(o["out_off"], np.concatenate([[0], np.cumsum(led.rec_u)]), err_msg=what)
    assert not o["flags"].any(), what
    # the ledger is the image's 91 8d 4c set (Layout.finish asserted it too), each with the right claim
    np.testing.assert_array_equal(SC.magic_positions(img), led.mag_pos, err_msg=what)
    np.testing.assert_array_equal(SC.frames_in_image(img, led.mag_pos), led.mag_frames, err_msg=what)
    live = led.mag_pos[led.mag_chain]
    np.testing.assert_array_equal(live, led.rec_off if led.stop == SC.NONE or not len(live) or live[-1] != led.stop
                                  else np.append(led.rec_off, led.stop), err_msg=what)
    # the tree the case is named for
    n_chunks, n_blocks, n_tiles = SC.geometry(len(img))
    assert n_chunks == case.n_chunks == m["n_chunks"], (what, n_chunks)
    if case.group.startswith("N") and "-" not in case.group:
        assert n_chunks == int(case.group[1:]), what
    # the event's chunk, and whether it is that chunk's first record start
    if case.cstar is not None:
        assert led.event != SC.NONE and (led.event - SC.HDR) // SC.CB == case.cstar, (what, led.event)
        assert m["arrive"][case.cstar] != SC.NONE, what
        assert (m["arrive"][case.cstar] == led.event) == (case.how == "first"), (what, m["arrive"][case.cstar])
    # the engineered repair count and path
    if case.repairs is not None:
        op, k = case.repairs
        r = m["expected_repairs"]
        assert (r == k) if op == "eq" else (r >= k), (what, r)
    if case.fast is not None:
        assert m["must_be_fast"] == case.fast, what
    if m["must_be_fast"]:  # nothing frames anywhere off the chain
        assert led.mag_chain[led.mag_frames].all(), what
    # placement: chunk c's records are the file's records [base_idx, base_idx + owned), the ones that start in it, and
    # base_bytes is where the first of them decodes to
    assert int(m["owned"].sum()) == o["n_records"], what
    np.testing.assert_array_equal(np.repeat(np.arange(n_chunks), m["owned"]), (o["rec_off"] - SC.HDR) // SC.CB, err_msg=what)
    np.testing.assert_array_equal(m["base_bytes"], o["out_off"][m["base_idx"]], err_msg=what)
    return n_chunks, n_blocks, n_tiles


@pytest.mark.parametrize("group", GROUP_IDS)
def test_case_is_what_it_claims(group):
    for case in SC.GROUPS[group]:
        check_case(case)


def test_the_trees_reach_their_level_2_paths():
    path = lambda n: SC.level2_path(SC.geometry(SC.cs(n))[1])  # noqa: E731
    assert SC.geometry(SC.cs(SC.N1))[1:] == (3, 1) and path(SC.N1) == "one wave"
    assert SC.geometry(SC.cs(SC.N2))[1:] == (67, 1) and path(SC.N2) == "tiled"
    assert SC.geometry(SC.cs(SC.N3))[1:] == (259, 2) and path(SC.N3) == "tiled"
    assert path(16384) == "one wave" and path(16385) == "tiled"
    assert SC.geometry(SC.cs(65536))[2] == 1 and SC.geometry(SC.cs(65537))[2] == 2
    # the events stand at the first and last chunk of a block, of the 64-block switch and of a tile
    for n, positions in SC.TREES.values():
        assert all(c in (0, 1, n - 1) or c % SC.BLOCK in (0, SC.BLOCK - 1) for c in positions)
    assert SC.SPAN_A[1] % SC.BLOCK == 0 and SC.geometry(SC.cs(SC.SPAN_C[2]))[2] == 3


def test_every_kind_stands_at_every_position():
    for tree, (n, positions) in SC.TREES.items():
        for c in positions:
            for kind in SC.KINDS:
                if kind == "false_on_chain" and c == 0:
                    continue  # nothing precedes chunk 0, and its entry is forced to 8
                assert f"{tree}-c{c}-{kind}" in SC.GROUPS, (tree, c, kind)


def test_rec_total_is_exact():
    for total in list(range(SC.MIN_REC, 300)) + [16394, 16395, 16396, 16397, 1 << 22]:
        r = SC.rec_total(total)
        assert len(r) == total
        img = np.frombuffer(b"\x04\x00\x00\x00\x00\x00\x00\x00" + r, np.uint8)
        o = orc.file_reader_decode_arrays(img)
        assert (o["n_records"], o["status"], o["total_out_bytes"]) == (1, STATUS["EOF"], SC.split_total(total)[0]), total
    assert len(SC.header(127, 1)) == 11 and len(SC.header(128, 2)) == 12
