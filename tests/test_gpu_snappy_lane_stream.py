"""The Snappy lane decoder streaming several records per lane (snappy_lane<kMulti = true>), on the GPU.

A lane that holds several records decodes them as one stream: at a record's end it switches to the
next record's descriptor, fetched in the slot a far-history load would use, and the copy window
restarts at the new record's first byte while the old record's bytes are still in the lane's history.
Both launch sites take that instantiation only from two records per lane on (k_snappy_pipe from
2 097 152 records, k_snappy_pipe_batch from 131 073 in a batch), so the files here are tiled
(tests/snappy_streams.py: every ordered pair of record forms adjacent inside a lane, every form
first, in the middle and last in a lane, valid and invalid) and counted to land there;
tests/test_snappy_streams_host.py proves that they do, from tests/lane_split.py. Every case is the
device result against the oracle's FileReader loop: status, counts, rec_off, out_off, flags,
first_bad, n_bad, and every byte outside the records the oracle flags.
"""
import numpy as np
import pytest

import oracle_py as orc
import snappy_streams as S
from gpu_util import assert_same_as_oracle, decoder, gpu_decode_arrays
from lane_split import batch_split, pipe_split
from recordio import _lib as L
from recordio import generate
from recordio.device import to_device_file

pytestmark = pytest.mark.gpu


def _host(b, info):
    k, nb = info["n_records"], info["total_out_bytes"]
    return dict(info, out=b.out[:nb].cpu().numpy(), out_off=b.out_off[:k + 1].cpu().numpy(),
                rec_off=b.rec_off[:k].cpu().numpy(), flags=b.flags[:k].cpu().numpy())


@pytest.fixture(scope="module")
def tiled():
    """The files of a case of snappy_streams.CASES, built once for the module."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = S.case_tiles(name)
        return made[name]

    return get


def check_batch(tiles, name, others=()):
    """One decode_batch of the case's tiled files and `others` (files the lane decoder leaves alone),
    every file against the oracle."""
    per = S.CASES[name][0]
    assert batch_split([t.n for t in tiles])[0] == per
    images = [t.image for t in tiles] + list(others)
    got = decoder().decode_batch([to_device_file(img) for img in images])
    assert len(got) == len(images)
    for k, (img, (b, info)) in enumerate(zip(images, got)):
        o = orc.file_reader_decode_arrays(img)
        assert o["status"] == L.RIO_EOF
        if k < len(tiles):
            assert o["n_records"] == tiles[k].n and o["n_bad"] == tiles[k].n_invalid
        assert_same_as_oracle(_host(b, info), o, f"{name}[{k}]")


@pytest.mark.parametrize("rpl", [2, 3, 5])
def test_batch_records_per_lane(tiled, rpl):
    """Valid forms only, three files of uneven size; the uncompressed file shares the launch group
    and must not count towards the records the lanes are dealt."""
    check_batch(tiled(f"rpl{rpl}"), f"rpl{rpl}", [generate(500, 200, 0, kind=0, seed=rpl).tobytes()])


def test_batch_records_per_lane_raised_for_the_wave_count(tiled):
    """15 files of 65 records and one of 130 000: one record per lane would need 2062 waves."""
    check_batch(tiled("need"), "need")


def test_batch_failing_lanes_listed(tiled):
    """Invalid records in at most 1024 lanes per file: finish_file decodes the listed lanes' records
    again, and every good record that shares a lane with a bad one is exact."""
    check_batch(tiled("listed"), "listed")


def test_batch_failing_lanes_overflow(tiled):
    """More failing lanes than the list holds: finish_file goes over every record."""
    check_batch(tiled("overflow"), "overflow")


@pytest.mark.parametrize("name", ["single_rpc2", "single_rpc2_overflow"])
def test_single_file_two_records_per_lane(tiled, name):
    """rio_device_decode of 2 097 152 + 4097 records, valid and invalid forms: k_snappy_pipe's
    kMulti instantiation (rpc = 2). In the first file at most 1024 lanes fail, so finish_file decodes
    only those again and every other record is as the lane decoder left it; in the second the list
    overflows and finish_file goes over every record."""
    (t,) = tiled(name)
    assert pipe_split(t.n)[0] == 2
    o = orc.file_reader_decode_arrays(t.image)
    assert o["status"] == L.RIO_EOF and o["n_records"] == t.n and o["n_bad"] == t.n_invalid
    assert_same_as_oracle(gpu_decode_arrays(t.image), o, name)


def test_ring_far_boundary_in_the_one_record_loop():
    """Copies of every offset 225..240 (kFarOff = 232: the last offset the LDS history serves) at
    every destination alignment and the lengths around one piece, one record per lane
    (snappy_lane<false, ...>); record 0 copies from the arena's first bytes."""
    import random

    sts = [S.far_from_start_stream(random.Random(5))] + S.edge_matrix()
    img = S.file_of(sts)
    assert pipe_split(len(sts))[0] == 1
    o = orc.file_reader_decode_arrays(img)
    assert o["status"] == L.RIO_EOF and o["n_records"] == len(sts) and o["n_bad"] == 0
    assert_same_as_oracle(gpu_decode_arrays(img), o, "edge matrix")


def test_batch_equals_single_calls(tiled):
    """The files of the rpl = 2 batch, decoded one per call (one record per lane), give the batch's bytes."""
    tiles = tiled("rpl2")
    files = [to_device_file(t.image) for t in tiles]
    batch = decoder().decode_batch(files)
    for (d, n), (b, info) in zip(files, batch):
        b1, i1 = decoder().decode(d, n)
        assert info["status"] == i1["status"] == L.RIO_EOF and info["n_records"] == i1["n_records"]
        nb = info["total_out_bytes"]
        assert nb == i1["total_out_bytes"]
        assert np.array_equal(b.out[:nb].cpu().numpy(), b1.out[:nb].cpu().numpy())
        assert np.array_equal(b.out_off.cpu().numpy(), b1.out_off.cpu().numpy())
        assert np.array_equal(b.flags.cpu().numpy(), b1.flags.cpu().numpy())
