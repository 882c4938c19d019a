"""k_sst_validate on built arrays (GPU): CRC-64/ISO at every length class and source alignment, the two
atomicMin results, and the layout search, through rio_sst_validate and rio_sst_validate_view.

The model is plain Python: a dict from record offset to record number (MMapReader.ReadNextAt at a record's
start), the oracle's CRC-64/ISO of that record's value, 0 as "no checksum". An entry whose valueOffset is no
record's offset gets CRC 0 and no checksum comparison (include/rio.h). Arrays are well formed throughout:
ascending offsets that end at the arena's length, RIO_DEVICE_PAD bytes of slack behind the arena."""
import random

import numpy as np
import pytest

import oracle_py as orc
import sst_wire_cases as W
from recordio import _lib as L
from test_gpu_sst_wire import BIG_N, LANES, NONE, ROUND, arena_of, data_entries, offsets, to_device, u64

pytestmark = pytest.mark.gpu

TOP = 1 << 63


def i64(a):
    import torch

    a = np.ascontiguousarray(np.asarray(a, dtype=np.uint64))
    return torch.from_numpy(a.view(np.int64).copy() if len(a) else np.zeros(1, dtype=np.int64)).cuda()


def validate(arena, off, rec_off, value_off, checksum, view=None):
    """rio_sst_validate (rio_sst_validate_view with `view`) -> (crc_out, [result0, result1])"""
    import torch

    n_data, n_index = len(off) - 1, len(value_off)
    d, doff = to_device(arena, off)
    drec, dvo, dcs = i64(rec_off), i64(value_off), i64(checksum)
    crc = torch.full((max(n_index, 1),), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda:0")
    res = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    lib, ctx = L.lib(), L.default_ctx(0)
    if view is None:
        rc = lib.rio_sst_validate(ctx, d.data_ptr(), doff.data_ptr(), drec.data_ptr(), n_data, dvo.data_ptr(),
                                  dcs.data_ptr(), n_index, crc.data_ptr(), res.data_ptr(), None)
    else:
        dview = i64(np.asarray(view, dtype=np.uint64).reshape(-1))
        rc = lib.rio_sst_validate_view(ctx, d.data_ptr(), doff.data_ptr(), drec.data_ptr(), n_data, dview.data_ptr(),
                                       dvo.data_ptr(), dcs.data_ptr(), n_index, crc.data_ptr(), res.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return u64(crc)[:n_index], [int(x) for x in u64(res)]


def model(values, rec_off, value_off, checksum):
    """values[j]: what record j hashes as -> (crc per entry, [first mismatch, first entry out of layout])"""
    at = {int(o): j for j, o in enumerate(rec_off)}
    crcs, first_bad, unplaced = [], NONE, NONE
    for i, (vo, cs) in enumerate(zip(value_off, checksum)):
        j = at.get(int(vo))
        if j != i:
            unplaced = min(unplaced, i)
        if j is None:
            crcs.append(0)
            continue
        c = orc.crc64_iso(values[j])
        crcs.append(c)
        if cs != 0 and c != cs:
            first_bad = min(first_bad, i)
    return crcs, [first_bad, unplaced]


def check(values, rec_off, value_off, checksum, want_result=None):
    arena, off = arena_of(values)
    crc, res = validate(arena, off, rec_off, value_off, checksum)
    want_crc, want_res = model(values, rec_off, value_off, checksum)
    assert crc.tolist() == want_crc
    assert res == want_res
    if want_result is not None:
        assert res == want_result
    return crc.tolist()


def record_offsets(n, rng):
    """Ascending file offsets as a writer's records have them: irregular gaps, the first behind a file header."""
    return np.cumsum([8] + [rng.randint(5, 300) for _ in range(n - 1)]).astype(np.uint64) if n else np.zeros(0, np.uint64)


LENGTHS = list(range(131)) + [191, 192, 193, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]


def test_every_length_class_at_every_alignment():
    """Every value length around the 16- and 64-byte loops of crc64_value, each starting at every address mod 16:
    a filler record of random bytes before each value sets its alignment. One launch."""
    rng = random.Random(64)
    values, checked = [], []
    pos = 0
    for n in LENGTHS:
        for a in range(16):
            gap = (a - pos) % 16 or 16
            values.append(rng.randbytes(gap))
            pos += gap
            assert pos % 16 == a
            checked.append(len(values))
            values.append(rng.randbytes(n))
            pos += n
    rec_off = record_offsets(len(values), rng)
    sums = [orc.crc64_iso(v) for v in values]
    assert sum(1 for j in checked if sums[j] & TOP) > 500 and sum(1 for j in checked if not sums[j] & TOP) > 500
    got = check(values, rec_off, rec_off, sums, [NONE, NONE])
    assert got == sums and len(checked) == 16 * len(LENGTHS)


def small_table(n, seed):
    rng = random.Random(seed)
    values = [rng.randbytes(rng.choice((1, 7, 8, 15, 16, 17, 40, 64, 65))) for _ in range(n)]
    values[20] = values[n // 2 + 1] = b""
    return values, record_offsets(n, rng), [orc.crc64_iso(v) for v in values]


def test_zero_checksum_is_unchecked():
    values, rec_off, sums = small_table(600, 1)
    stored = list(sums)
    stored[5] = 0
    stored[300] = 0
    check(values, rec_off, rec_off, stored, [NONE, NONE])
    stored[301] = sums[301] ^ 1  # beside a wrong one
    check(values, rec_off, rec_off, stored, [301, NONE])


@pytest.mark.parametrize("flip_low,flip_high", [(0xFF << 56, 0xFF), (0xFF, 0xFF << 56), (TOP, 1), (1, TOP)])
def test_first_of_two_mismatches_in_different_blocks(flip_low, flip_high):
    """Stored checksums that differ from the value's CRC in the top byte only or in the low byte only, at entries 3
    and 700 (blocks 0 and 2) and the other way round: the smaller index is reported."""
    values, rec_off, sums = small_table(900, 2)
    assert 3 // LANES != 700 // LANES
    stored = list(sums)
    stored[3] ^= flip_low
    stored[700] ^= flip_high
    assert stored[3] and stored[700]
    check(values, rec_off, rec_off, stored, [3, NONE])
    stored[3] = sums[3]
    check(values, rec_off, rec_off, stored, [700, NONE])


def test_entry_pointing_at_another_record():
    values, rec_off, sums = small_table(600, 3)
    for i, j in ((10, 11), (400, 2), (2, 599), (599, 0)):
        assert sums[i] != sums[j]
        vo, stored = list(rec_off), list(sums)
        vo[i] = rec_off[j]
        got = check(values, rec_off, vo, stored, [i, i])  # record j's CRC against entry i's checksum
        assert got[i] == sums[j]
        stored[i] = sums[j]
        check(values, rec_off, vo, stored, [NONE, i])
        stored[i] = 0
        check(values, rec_off, vo, stored, [NONE, i])


def test_value_offset_that_is_no_record():
    values, rec_off, sums = small_table(600, 4)
    assert rec_off[0] > 0 and rec_off[301] - rec_off[300] > 1
    for i, off in ((7, 0), (7, int(rec_off[0]) - 1), (300, int(rec_off[300]) + 1), (300, int(rec_off[301]) - 1),
                   (599, int(rec_off[599]) + 1), (0, NONE), (599, NONE), (258, NONE - 1)):
        vo = [int(x) for x in rec_off]
        vo[i] = off
        got = check(values, rec_off, vo, sums, [NONE, i])  # CRC 0, and the non-zero checksum is not compared
        assert got[i] == 0 and sums[i] != 0


def test_first_of_two_out_of_layout_entries_in_different_blocks():
    values, rec_off, sums = small_table(900, 5)
    for low, high in ((int(rec_off[9]), NONE), (NONE, int(rec_off[9])), (1, int(rec_off[0]))):
        vo = [int(x) for x in rec_off]
        vo[3], vo[700] = low, high
        check(values, rec_off, vo, [0] * 900, [NONE, 3])
        vo[3] = int(rec_off[3])
        check(values, rec_off, vo, [0] * 900, [NONE, 700])


def test_more_index_entries_than_records():
    values, rec_off, sums = small_table(300, 6)
    vo = [int(x) for x in rec_off] + [int(rec_off[j]) for j in (0, 299, 150)] + [int(rec_off[299]) + 1]
    stored = sums + [sums[0], sums[299], sums[150] ^ TOP, 12345]
    got = check(values, rec_off, vo, stored, [302, 300])  # entries past n_data take the search
    assert got[300:] == [sums[0], sums[299], sums[150], 0]


def test_fewer_index_entries_than_records():
    values, rec_off, sums = small_table(600, 7)
    check(values, rec_off, rec_off[:257], sums[:257], [NONE, NONE])
    stored = sums[:257]
    stored[256] ^= 1 << 32
    check(values, rec_off, rec_off[:257], stored, [256, NONE])


def test_no_records_and_no_entries():
    got = check([], np.zeros(0, np.uint64), [8, 0, NONE], [1, 2, 3], [NONE, 0])
    assert got == [0, 0, 0]
    values, rec_off, sums = small_table(30, 8)
    check(values, rec_off, [], [], [NONE, NONE])


def test_validate_view_ranges():
    """rio_sst_validate_view over the ranges rio_sst_data_entries gives for valid, nil and malformed DataEntry
    records: a nil or malformed value hashes as the empty value, so a stored checksum on it is a mismatch; values
    begin at every address mod 16 (junk fields of every length before them)."""
    rng = random.Random(9)
    records, pos = [], 0
    for n in (0, 1, 15, 16, 17, 63, 64, 65, 130, 1025):
        for a in range(16):
            head = 2 + 1 + len(W.uv(n))  # the junk field's tag and length, the value's tag and length
            junk = (a - pos - head) % 16
            records.append(W.field(9, bytes(junk)) + W.field(1, rng.randbytes(n)) + W.field(2, 7, 0))
            assert (pos + head + junk) % 16 == a
            pos += len(records[-1])
        records += [r for _, r in W.data_family()[n % 7::7]]
        pos = sum(len(r) for r in records)
    means = [W.data_entry_model(r) for r in records]
    nil, bad = means.index(None), means.index(W.BAD)
    arena, off = arena_of(records)
    view, first = data_entries(arena, off)
    assert first == bad
    begins = {int(view[j, 0]) % 16 for j, m in enumerate(means) if isinstance(m, bytes) and len(m) >= 64}
    assert begins == set(range(16))
    hashed = [m if isinstance(m, bytes) else b"" for m in means]
    sums = [orc.crc64_iso(v) for v in hashed]
    assert orc.crc64_iso(b"") == 0
    rec_off = record_offsets(len(records), rng)

    def run(value_off, stored, want):
        crc, res = validate(arena, off, rec_off, value_off, stored, view)
        want_crc, want_res = model(hashed, rec_off, value_off, stored)
        assert crc.tolist() == want_crc and res == want_res == want

    run(rec_off, sums, [NONE, NONE])
    for j in sorted((nil, bad)):
        stored = list(sums)
        stored[j] = 77
        run(rec_off, stored, [j, NONE])
    vo = [int(x) for x in rec_off]
    vo[nil] = int(rec_off[bad])
    vo[5] = int(rec_off[5]) + 1
    run(vo, sums, [NONE, min(nil, 5)])


def test_beyond_one_round_of_the_grid():
    """One round of the grid and 257 entries more: values of 0..7 bytes from 256 distinct ones, the one mismatch and
    the one out-of-layout entry beyond the first round."""
    rng = np.random.default_rng(11)
    rows = rng.integers(0, 256, size=(256, 8), dtype=np.uint8)
    row_len = np.arange(256) % 8
    row_crc = np.array([orc.crc64_iso(rows[k, :row_len[k]].tobytes()) for k in range(256)], dtype=np.uint64)
    ids = rng.integers(0, 256, size=BIG_N)
    lens = row_len[ids].astype(np.uint64)
    arena = rows[ids][np.arange(8)[None, :] < lens[:, None].astype(np.int64)]
    off = offsets(lens)
    rec_off = off[:-1] + np.uint64(9) * np.arange(BIG_N, dtype=np.uint64) + np.uint64(8)
    value_off, stored, want = rec_off.copy(), row_crc[ids].copy(), row_crc[ids].copy()
    wrong, moved = ROUND + 50, ROUND + 200
    stored[wrong] ^= np.uint64(1)
    value_off[moved] = rec_off[5]
    want[moved] = stored[moved] = row_crc[ids[5]]
    crc, res = validate(arena, off, rec_off, value_off, stored)
    assert res == [wrong, moved]
    np.testing.assert_array_equal(crc, want)
