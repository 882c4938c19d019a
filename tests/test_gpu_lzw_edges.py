"""Crafted lzw streams (tests/lzw_model.py) on the device vs the oracle (GPU): a full table without a
clear (k_lzw_decode's `hi = min(257 + k, 4095)`, its 3840-entry table and closed-form bit positions
past code 3838), code == hi at the width steps, KwKwK chains across rounds, copies at the 64-byte
output windows, and the small class's 16-bit positions at 65535 / 65536 decoded bytes. The device
must equal the oracle, never hand back, and for valid streams equal what the Python model of Go's
reader decodes (tests/test_lzw_model.py ties the model and the oracle together on the CPU)."""
import numpy as np
import pytest

import corpus
import lzw_model as M
import oracle_py as orc
from conftest import STATUS
from gpu_util import assert_same_as_oracle, gpu_decode_arrays

pytestmark = pytest.mark.gpu


def edge_file(name):
    return next(f for f in M.files() if f[0] == name)


def check(g, image, expect, what):
    assert g["status"] != STATUS["UNSUPPORTED"], what
    assert_same_as_oracle(g, orc.file_reader_decode_arrays(image), what)
    assert g["n_records"] == len(expect), what
    for i, want in enumerate(expect):
        if want is M.CORRUPT:
            assert g["flags"][i] & 2, (what, i)
        else:
            assert not g["flags"][i] & 6, (what, i)
            assert bytes(g["out"][g["out_off"][i]:g["out_off"][i + 1]]) == want, (what, i)


@pytest.mark.parametrize("name", M.FILE_NAMES)
def test_lzw_edges_on_the_device(name):
    _, image, expect = edge_file(name)
    check(gpu_decode_arrays(image), image, expect, name)


def test_lzw_edges_through_the_host_api():
    import ctypes

    from recordio import _lib as L
    from test_gpu_threads import host_decode

    name, image, expect = edge_file(M.FILE_NAMES[-1])
    h = ctypes.c_void_p()
    assert L.lib().rio_ctx_create(0, ctypes.byref(h)) == 0
    try:
        g = host_decode(h.value, np.frombuffer(image, dtype=np.uint8))
    finally:
        L.lib().rio_ctx_destroy(h)
    check(g, image, expect, name + " host api")


def test_lzw_edges_in_a_batch():
    from recordio import generate
    from recordio.device import to_device_file
    from gpu_util import decoder

    imgs = [generate(500, 300, 2, kind=1, seed=9).tobytes()] + [f[1] for f in M.files()]
    got = decoder().decode_batch([to_device_file(i) for i in imgs])
    for k, (img, (b, info)) in enumerate(zip(imgs, got)):
        n, nb = info["n_records"], info["total_out_bytes"]
        g = dict(info, out=b.out[:nb].cpu().numpy(), out_off=b.out_off[:n + 1].cpu().numpy(),
                 rec_off=b.rec_off[:n].cpu().numpy(), flags=b.flags[:n].cpu().numpy())
        if k:
            check(g, img, M.files()[k - 1][2], f"batch {k}")
        else:
            assert_same_as_oracle(g, orc.file_reader_decode_arrays(img), "batch snappy")


# ---- launch shapes: one grid plus three records (csrc/rio_lzw.hip: kLzSmallGrid = 256 * 32 one-wave
# workgroups for payloads <= kLzSmallLen = 1152 bytes decoding to < 65536; kLzGrid = 1536 for the rest) ----
SMALL_GRID, LARGE_GRID, SMALL_LEN = 256 * 32, 1536, 1152


@pytest.mark.parametrize("grid,lo,hi,letters", [(SMALL_GRID, 200, 600, 8), (LARGE_GRID, 1500, 1700, 256)],
                         ids=["small", "large"])
def test_grid_stride_loops_take_a_second_turn(grid, lo, hi, letters):
    n = grid + 3
    rng = np.random.default_rng(grid)
    lens = rng.integers(lo, hi + 1, size=n)
    pool = rng.integers(0, letters, size=int(lens.sum()), dtype=np.uint8).tobytes()
    recs, p = [], 0
    for i, ln in enumerate(lens.tolist()):
        recs.append((b"%d:" % i + pool[p:p + ln])[:ln])
        p += ln
    assert len(set(recs)) == n
    pays = [orc.lzw_encode(r) for r in recs]
    assert all((len(q) <= SMALL_LEN) == (grid == SMALL_GRID) for q in pays)
    items = [(len(r), q) for r, q in zip(recs, pays)]
    bad = grid + 1  # truncated (io.ErrUnexpectedEOF) at an index only the loop's second turn reaches
    items[bad] = (items[bad][0], items[bad][1][:-2])
    image = corpus.lzw_file(items)
    o = orc.file_reader_decode_arrays(image)
    assert o["n_records"] == n and o["n_bad"] == 1 and o["first_bad"] == bad
    g = gpu_decode_arrays(image)
    assert g["status"] != STATUS["UNSUPPORTED"]
    assert_same_as_oracle(g, o, f"launch {n}")
    for k in (0, grid - 1, grid, grid + 2, n - 1):
        assert bytes(g["out"][g["out_off"][k]:g["out_off"][k + 1]]) == recs[k], k


# ---- the resize round per framing chunk: k_lzw_resize walks the chunks on kLzGrid = 1536 one-wave
# workgroups (`c += gridDim.x`) and corrects scratch_len / chunks[c].bytes of the chunk a record is in ----
@pytest.mark.parametrize("chunk", [None, 256, 4096], ids=["default", "256", "4096"])
def test_resize_round_per_chunk(chunk, monkeypatch, capsys):
    """Every 50th header's u is 7 off the decoded length. At the default chunk size the result is the
    oracle's outright; at 256 bytes (more than 1536 chunks: the loop's second turn) and 4096 the
    documented hand-back at a record that needs the redo round is accepted, everything before it exact."""
    from gpu_util import assert_exact_or_handed_back_at, decode_in_new_context

    image, recs, redo = M.redo_file()
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
        print(f"\n[lzw resize round, chunk {chunk or 'default'}: {how}, repairs {g.get('n_repairs')}]")
    for k in (0, 48, 49, 50):
        if k < g["n_records"]:
            assert bytes(g["out"][g["out_off"][k]:g["out_off"][k + 1]]) == recs[k], k


@pytest.mark.parametrize("chunk", [None, 256], ids=["default", "256"])
def test_resize_round_after_a_sequential_repair(chunk, monkeypatch, capsys):
    """Payloads that hold recordio files break the chunk speculation (n_repairs > 0), so the placement
    is the sequential repair's: the resize kernel then hands the file back at the first record that
    needs the redo round (`st->slow`), or the result is exact; nothing else is accepted."""
    from gpu_util import assert_exact_or_handed_back_at, decode_in_new_context

    image, recs, redo = M.embedded_redo_file()
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
        print(f"\n[lzw resize round after a repair, chunk {chunk or 'default'}: {how}, repairs {g['n_repairs']}]")
    for k in range(min(g["n_records"], len(recs))):
        assert bytes(g["out"][g["out_off"][k]:g["out_off"][k + 1]]) == recs[k], k
