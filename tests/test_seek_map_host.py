"""The SeekNext map's model against the oracle's SeekNext, and the case families against what they
are there to contain (CPU).

tests/seek_map_model.py restates the map from mmap_reader.go:58-128. Here every position's end in the
model is what the oracle's SeekNext from that position says: the decoded record whose offset it
returns, io.EOF, or a trial offset that is no decoded record start. The two large families (the
multi-megabyte `segments` files and the 270 001-byte run) are checked at every position within 8 bytes of
a segment boundary and at 500 seeded ones. tests/test_gpu_seek_map.py then holds the device's P / R to
the model on the same files.
"""
import numpy as np
import pytest

import seek_map_model as M

NAMES = M.all_names()
IDS = [n for _, n in NAMES]


def _large(fam, name):
    return fam in M.LARGE or name in M.LARGE


@pytest.mark.parametrize("fam,name", NAMES, ids=IDS)
def test_model_end_is_the_oracles_seek_next(fam, name):
    raw, rec_off, P, R, _ = M.solved(fam, name)
    if len(raw) < 8:  # no file header: SeekNext has no file to scan
        assert P.shape[0] == 0
        return
    rec_at = {o: j for j, o in enumerate(rec_off)}
    ks = M.sample(fam, name) if _large(fam, name) else range(P.shape[0])
    bad = [(k, int(P[k]), int(R[k]), w) for k in ks if (w := M.oracle_end(raw, rec_at, int(P[k]))) != int(R[k])]
    assert not bad, (len(bad), bad[:5])
    # before the first 0x91 and behind the last: the first position's answer, and io.EOF
    if P.shape[0]:
        assert M.oracle_end(raw, rec_at, 0) == int(R[0])
        assert M.oracle_end(raw, rec_at, int(P[-1]) + 1) == M.EOF
    else:
        assert M.oracle_end(raw, rec_at, 0) == M.EOF


@pytest.mark.parametrize("fam,name", [x for x in NAMES if x[0] in ("boundaries", "ends")],
                         ids=[n for f, n in NAMES if f in ("boundaries", "ends")])
def test_answer_is_fixed_by_the_next_0x91_at_every_window_size(fam, name):
    """The claim the map rests on: with windows of 4 bytes or more, SeekNext from the byte behind the
    previous 0x91 and from the 0x91 itself give one answer, whatever the window."""
    raw, _, P, _, _ = M.solved(fam, name)
    if len(raw) < 8:
        return
    for k in range(P.shape[0]):
        want = M.seek_next(raw, int(P[k]), 4096)
        lo = int(P[k - 1]) + 1 if k else 0
        for seek_len in (4, 5, 64, 4096):
            for off in {lo, int(P[k])}:
                assert M.seek_next(raw, off, seek_len) == want, (name, k, off, seek_len)


# ------------------------------------------------------------------------------------------------
# what each family is there to contain
# ------------------------------------------------------------------------------------------------
def test_boundaries_split_a_marker_both_ways_at_every_boundary_kind():
    files = M.family("boundaries")
    assert len(files) == len(M.ITEMS) * len(M.DELTAS)
    for item, blob in M.ITEMS.items():
        for d in M.DELTAS:
            raw = files[f"bnd_{item}_{d:+d}"]
            for _, at in M.boundary_places(d):
                assert raw[at:at + len(blob)] == blob
            assert (len(raw) - 1) // M.SEG * M.SEG == M.boundary_places(0)[3][1]  # "last" is the last segment's start
    assert M.B16 % 16 == 0 and M.B16 % 64 and M.B64 % 64 == 0 and M.B64 % 4096 and M.B4096 % 4096 == 0
    # 1 | 2 and 2 | 1 bytes of a marker (d = -1, -2), 1 | 1 of `91 8d`, and the 0x91 byte as the last and
    # the first of its unit, at a multiple of 16 only, of 64 only, of 4096, and at the last segment's start
    for kind, at in M.boundary_places(0):
        unit = 4096 if kind == "last" else kind
        for item in ("dead", "live"):
            starts = {p + d for d in M.DELTAS for k, p in M.boundary_places(0) if k == kind}
            assert {at - 1, at - 2} <= starts and (at - 1) % unit == unit - 1 and (at - 2) % unit == unit - 2, item
    # the filler holds no 0x91: every position is a placed item's or a record header's
    raw, rec_off, P, _, _ = M.solved("boundaries", "bnd_lone_+0")
    placed = {at for _, at in M.boundary_places(0)}
    in_header = {o + i for o in rec_off for i in range(12)}  # (a header's CRC varint may hold one too)
    assert placed <= set(P.tolist()) and set(P.tolist()) - placed <= in_header and len(rec_off) > 12


def test_tails_cover_every_residue_and_tail():
    files = M.family("tails")
    mods = {}
    for name, raw in files.items():
        if name.startswith("tail_mod"):
            mods[len(raw) % 16] = next(t for t in reversed(M.TAILS) if raw.endswith(t))
    assert sorted(mods) == list(range(16)) and set(mods.values()) == set(M.TAILS)
    assert len(files["tail_2seg_exact"]) == 2 * M.SEG and files["tail_2seg_exact"][-1] == 0x91
    for name in files:  # the cut marker is the last position, and its walk is io.EOF
        _, _, P, R, _ = M.solved("tails", name)
        assert int(R[-1]) == M.EOF


def test_segments_reach_the_scans_per_values():
    per = {n: (n + 1023) // 1024 for n in M.SEGMENT_COUNTS}
    assert per[1024] == 1 and per[1025] == per[1027] == 2 and per[2049] == 3
    assert 1023 * per[2049] > 2049  # k_scan_segs: the last threads' first index lies past n
    assert 1027 % 4 and 2049 % 4 and 1023 % 4 and 1024 % 4 == 0
    for n in M.SEGMENT_COUNTS:
        raw, rec_off, P, R, _ = M.solved("segments", f"seg_{n}")
        assert (len(raw) + M.SEG - 1) // M.SEG == n and len(raw) % 16
        seg = (P // np.uint64(M.SEG)).astype(np.int64)
        assert set(seg.tolist()) == set(range(n))  # every segment holds a 0x91
        # the three last segments each hold a lane of 64 0x91 bytes
        for s in range(max(n - 3, 0), n):
            lane = ((P[seg == s] % np.uint64(M.SEG)) // np.uint64(64)).astype(np.int64)
            assert np.bincount(lane).max() >= 64, (n, s)
        if n >= 64:  # the lane and the quarter rotate with the segment
            lanes = {int(p % M.SEG) // 64 for p in P.tolist()}
            quarters = {int(p % 64) // 16 for p in P.tolist()}
            assert len(lanes) == 64 and quarters == {0, 1, 2, 3}
        assert len(rec_off) == (len(raw) + M.REC - 1) // (M.REC + 10) and set(R.tolist()) - {M.EOF, M.OTHER}


def test_chains_reach_the_second_grid_turn_and_eighteen_rounds():
    raw, _, P, R, steps = M.solved("chains", "chain_long_run")
    assert P.shape[0] > 1024 * 256  # k_seek_step / k_seek_jump: a second turn of the grid-stride loop
    assert steps.max() >= 1 << 17   # pointer jumping: 18 rounds
    # the two parities of the run end at the two records behind it
    k = int(np.searchsorted(P, raw.index(b"\x91" * 4)))
    assert {int(R[k]), int(R[k + 1])} == {1, 2} and int(R[k + 2]) == int(R[k])
    for g, Ls in M.CHAIN_GROUPS.items():
        for kind in ("runs", "trains"):
            raw, rec_off, P, R, steps = M.solved("chains", f"chain_{kind}_{g}")
            assert len(rec_off) == 4 * len(Ls)
            for i, L in enumerate(Ls):
                for h, n in enumerate((2 * L, 2 * L + 1)):
                    j = 4 * i + 2 * h  # the record holding the chain; j + 1 is the live one behind it
                    inside = np.flatnonzero((P > rec_off[j]) & (P < rec_off[j + 1]))
                    inside = inside[-n:]  # (the header before the chain may hold a 0x91 of its own)
                    got = set(R[inside].tolist())
                    if kind == "runs":  # one parity lands on the next marker, the other steps over it
                        want = {j + 1, j + 2} if j + 2 < len(rec_off) else {j + 1, M.EOF}
                        assert got == want and int(R[inside[-1]]) != j + 1, (g, L, n)
                        assert int(steps[inside[0]]) >= n // 2
                    else:  # every dead marker is passed: all end at the live record
                        assert got == {j + 1} and int(steps[inside[0]]) == n, (g, L, n)


def test_ends_hold_every_kind_of_end_and_file():
    kinds = {}
    for name in M.family("ends"):
        raw, rec_off, P, R, _ = M.solved("ends", name)
        kinds[name] = (len(rec_off), set(R.tolist()))
    for name in ("end_embedded_torn_eof", "end_embedded_torn_mid", "end_mid_break", "end_snappy", "end_gzip",
                 "end_lzw", "end_v3", "end_v2"):
        n, ends = kinds[name]
        assert n and ends & set(range(n)), name
    assert M.OTHER in kinds["end_embedded_torn_eof"][1] and M.EOF in kinds["end_embedded_torn_eof"][1]
    # a header torn after a whole varint is io.EOF and the walk runs out; torn inside one, the walk ends there
    raw, _, P, R, _ = M.solved("ends", "end_embedded_torn_eof")
    assert raw.endswith(b"\x91\x8d\x4c\x00\x05") and int(R[-1]) == M.EOF
    raw, _, P, R, _ = M.solved("ends", "end_embedded_torn_mid")
    assert raw.endswith(b"\x91\x8d\x4c\x00\x85") and int(R[-1]) == M.OTHER
    # a valid header whose payload passes the file end, and a CRC-failing one, are passed: the walk from each
    # ends where the walk from the next 0x91 does
    raw, _, P, R, _ = M.solved("ends", "end_embedded_torn_eof")
    for blob in (M.DEAD, b"\x91\x8d\x4c\x00\x80\x80\x40\x00"):
        k = int(np.searchsorted(P, raw.index(blob, 20)))
        assert int(P[k]) == raw.index(blob, 20) and int(R[k]) == int(R[k + 1])
    # 91 8d 91 8d 4c: the step from the first 0x91 passes the marker behind it
    at = raw.index(b"x\x91\x8d" + M.LIVE) + 1
    k = int(np.searchsorted(P, at))
    assert int(R[k]) != M.OTHER and int(R[k + 1]) == M.OTHER
    # behind the break every marker is outside the decoded sequence
    raw, rec_off, P, R, _ = M.solved("ends", "end_mid_break")
    assert len(rec_off) == 6 and set(R[P > rec_off[-1] + 12].tolist()) <= {M.OTHER, M.EOF}
    assert M.OTHER in set(R.tolist())
    # codec files: a corrupt record is a decoded record (its trial ends the walk with the codec's error);
    # gzip's empty payload is passed
    import oracle_py as orc
    for name in ("end_snappy", "end_gzip", "end_lzw"):
        o = orc.file_reader_decode(M.solved("ends", name)[0])
        assert None in o["records"] and orc.BadRecord("corrupt") in o["records"], name
        bad = o["records"].index(orc.BadRecord("corrupt"))
        assert bad in kinds[name][1], name
    o = orc.file_reader_decode(M.solved("ends", "end_gzip")[0])
    assert o["records"].index(orc.BadRecord("eof")) not in kinds["end_gzip"][1]
    assert kinds["end_header_only"] == (0, set()) and kinds["end_empty"] == (0, set())
    assert M.solved("ends", "end_v3")[0][0] == 3 and M.solved("ends", "end_v2")[0][0] == 2
