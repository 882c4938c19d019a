"""The hand-built DEFLATE families (tests/deflate_cases.py) on the device vs the oracle (GPU).

Each family is decoded as a file of small records by k_gzip_inflate (csrc/rio_gzip.hip); the result
must equal the oracle's (records, offsets, flags, status), never be handed back (UNSUPPORTED), and for
valid records equal the bytes the builder expanded from the tokens. Then every family shuffled into
one file (the tiny, small and large classes and the redo round in one decode), through the batch API
beside a Snappy file, and through the host pair rio_frame + rio_decode. The neighbour files put
records that fail at once, or run 100 times longer, beside ordinary ones in the four-records-per-wave
class. tests/test_deflate_cases.py shows on the CPU that the families are what they claim."""
import numpy as np
import pytest

import corpus
import deflate_cases as D
import oracle_py as orc
from conftest import STATUS
from gpu_util import assert_same_as_oracle, gpu_decode_arrays

pytestmark = pytest.mark.gpu

FAMILIES = [f.__name__ for f in D.VALID_FAMILIES + D.REFUSED_FAMILIES]  # the valid ones run first


def check(g, image, cases, what):
    assert g["status"] != STATUS["UNSUPPORTED"], what
    assert_same_as_oracle(g, orc.file_reader_decode_arrays(image), what)
    assert g["n_records"] == len(cases), what
    for i, c in enumerate(cases):
        if c is None:
            assert g["flags"][i] & 1, (what, i)
        elif c.valid:
            assert not g["flags"][i] & 6, (what, c.name)
            got = bytes(g["out"][g["out_off"][i]:g["out_off"][i + 1]])
            assert got == c.expect, (what, c.name)
        else:
            assert g["flags"][i] & 2, (what, c.name)


@pytest.mark.parametrize("name", FAMILIES)
def test_family_on_the_device(name):
    fam = D.cached(next(f for f in D.VALID_FAMILIES + D.REFUSED_FAMILIES if f.__name__ == name))
    for fname, image, cases in D.family_files(fam):
        check(gpu_decode_arrays(image), image, cases, fname)


def test_neighbours_four_records_per_wave():
    items = D.neighbour_family()
    image = corpus.gz_file([None if c is None else c.item for c in items])
    check(gpu_decode_arrays(image), image, items, "neighbours")


@pytest.fixture(scope="module")
def shuffled():
    return D.shuffled_all()


def test_all_families_shuffled_into_one_file(shuffled):
    image, cases = shuffled
    check(gpu_decode_arrays(image), image, cases, "shuffled")


def test_shuffled_file_in_a_batch_beside_snappy(shuffled):
    from recordio import generate
    from recordio.device import to_device_file
    from gpu_util import decoder

    image, cases = shuffled
    imgs = [generate(500, 300, 2, kind=1, seed=9).tobytes(), image]
    got = decoder().decode_batch([to_device_file(i) for i in imgs])
    for k, (img, (b, info)) in enumerate(zip(imgs, got)):
        n, nb = info["n_records"], info["total_out_bytes"]
        g = dict(info, out=b.out[:nb].cpu().numpy(), out_off=b.out_off[:n + 1].cpu().numpy(),
                 rec_off=b.rec_off[:n].cpu().numpy(), flags=b.flags[:n].cpu().numpy())
        if k == 1:
            check(g, img, cases, "batch")
        else:
            assert_same_as_oracle(g, orc.file_reader_decode_arrays(img), "batch snappy")


def test_shuffled_file_through_the_host_api(shuffled):
    import ctypes

    from recordio import _lib as L
    from test_gpu_threads import host_decode

    image, cases = shuffled
    h = ctypes.c_void_p()
    assert L.lib().rio_ctx_create(0, ctypes.byref(h)) == 0
    try:
        g = host_decode(h.value, np.frombuffer(image, dtype=np.uint8))
    finally:
        L.lib().rio_ctx_destroy(h)
    check(g, image, cases, "host api")


# ---- launch shapes: one grid plus a few records, so every grid-stride loop takes a second turn ----
# (csrc/rio_gzip.hip) gz_grid<kGzTinyWin>() = 256 * (8 / RIO_GZ_TW + 1) = 1280 workgroups of RIO_GZ_TW = 2
# waves, 64 / RIO_GZ_GROUP = 4 records per wave; gz_grid<kGzSmallWin>() = 1280 and gz_grid<kGzLargeWin>()
# = 256 workgroups of kGzWaves = 4 waves, one record per wave; launch_gzip_decode: k_gzip_crc on
# dim3(512) x dim3(256), one record per lane.
TINY_GROUPS, SMALL_WAVES, LARGE_WAVES, CRC_LANES = 1280 * 2 * 4, 1280 * 4, 256 * 4, 512 * 256


def distinct_records(n, lo, hi, seed):
    """n different text-like records of lo..hi bytes: the index, then letters from a small alphabet."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, size=n)
    pool = rng.integers(97, 105, size=int(lens.sum()), dtype=np.uint8).tobytes()
    out, p = [], 0
    for i, ln in enumerate(lens.tolist()):
        out.append((b"%d:" % i + pool[p:p + ln])[:ln])
        p += ln
    return out


@pytest.mark.parametrize("n,lo,hi,grid", [(TINY_GROUPS + 7, 20, 60, TINY_GROUPS), (SMALL_WAVES + 3, 1100, 2000, SMALL_WAVES),
                                          (LARGE_WAVES + 5, 2100, 2200, LARGE_WAVES), (CRC_LANES + 8, 8, 16, CRC_LANES)],
                         ids=["tiny", "small", "large", "crc"])
def test_grid_stride_loops_take_a_second_turn(n, lo, hi, grid):
    recs = distinct_records(n, lo, hi, n)
    assert n > grid and len(set(recs)) == n
    cls = lambda r: 0 if len(r) <= 1024 else 1 if len(r) <= 2048 else 2  # noqa: E731
    assert {cls(r) for r in recs} == {0 if hi <= 1024 else 1 if hi <= 2048 else 2}
    items = [(len(r), corpus.gzip_member(r, 1)) for r in recs]
    bad = grid + 2  # a wrong CRC-32 at an index only the loop's second turn reaches
    p = items[bad][1]
    items[bad] = (items[bad][0], p[:-8] + bytes([p[-8] ^ 1]) + p[-7:])
    image = corpus.gz_file(items)
    o = orc.file_reader_decode_arrays(image)
    assert o["n_records"] == n and o["n_bad"] == 1 and o["first_bad"] == bad
    g = gpu_decode_arrays(image)
    assert g["status"] != STATUS["UNSUPPORTED"]
    assert_same_as_oracle(g, o, f"launch {n}")
    for k in (0, grid - 1, grid, grid + 1, n - 2, n - 1):
        assert bytes(g["out"][g["out_off"][k]:g["out_off"][k + 1]]) == recs[k], k


# ---- the resize round per framing chunk: k_gz_resize walks the chunks (256 workgroups of kGzWaves = 4
# waves, `c += gridDim.x * kGzWaves`) and corrects scratch_len / chunks[c].bytes of the chunk a record is in ----
@pytest.mark.parametrize("chunk", [None, 256, 4096], ids=["default", "256", "4096"])
def test_resize_round_per_chunk(chunk, monkeypatch, capsys):
    """Every 50th record has two members. At the default chunk size the result is the oracle's outright;
    at 256 bytes (more than 1024 chunks: the loop's second turn) and 4096 the documented hand-back at a
    record that needs the redo round is accepted, with everything before it exact."""
    from gpu_util import assert_exact_or_handed_back_at, decode_in_new_context

    image, recs, redo = D.redo_file()
    if chunk is None:
        monkeypatch.delenv("RIO_CHUNK_BYTES", raising=False)
    else:
        monkeypatch.setenv("RIO_CHUNK_BYTES", str(chunk))
        assert len(image) > 1536 * 256
    o = orc.file_reader_decode_arrays(image)
    assert o["n_records"] == len(recs) and o["n_bad"] == 0
    g = decode_in_new_context(image)
    if chunk is None:
        assert g["status"] != STATUS["UNSUPPORTED"]
        assert_same_as_oracle(g, o, "redo default")
        how = "exact"
    else:
        how = assert_exact_or_handed_back_at(g, o, redo, f"redo@{chunk}")
    with capsys.disabled():
        print(f"\n[gzip resize round, chunk {chunk or 'default'}: {how}, repairs {g.get('n_repairs')}]")
    for k in (0, 48, 49, 50):
        if k < g["n_records"]:
            assert bytes(g["out"][g["out_off"][k]:g["out_off"][k + 1]]) == recs[k], k


@pytest.mark.parametrize("chunk", [None, 256], ids=["default", "256"])
def test_resize_round_after_a_sequential_repair(chunk, monkeypatch, capsys):
    """Payloads that hold recordio files break the chunk speculation (n_repairs > 0), so the placement
    is the sequential repair's: the resize kernel then hands the file back at the first record that
    needs the redo round (`st->slow`), or the result is exact; nothing else is accepted."""
    from gpu_util import assert_exact_or_handed_back_at, decode_in_new_context

    image, recs, redo = D.embedded_redo_file()
    if chunk is None:
        monkeypatch.delenv("RIO_CHUNK_BYTES", raising=False)
    else:
        monkeypatch.setenv("RIO_CHUNK_BYTES", str(chunk))
    o = orc.file_reader_decode_arrays(image)
    assert o["n_records"] == len(recs) and o["n_bad"] == 0
    g = decode_in_new_context(image)
    assert g["n_repairs"] > 0
    how = assert_exact_or_handed_back_at(g, o, redo, f"embedded redo@{chunk}")
    with capsys.disabled():
        print(f"\n[gzip resize round after a repair, chunk {chunk or 'default'}: {how}, repairs {g['n_repairs']}]")
    for k in range(min(g["n_records"], len(recs))):
        assert bytes(g["out"][g["out_off"][k]:g["out_off"][k + 1]]) == recs[k], k
