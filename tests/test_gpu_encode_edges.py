"""The device Snappy encoder (csrc/rio_encode.hip) at its tag, block and launch edges (GPU).

Expected bytes come from the oracle (oracle/rio_oracle.c, pinned to the reference writer's fixtures by
tests/test_writer.py); tests/test_encode_cases.py shows on the CPU that the oracle's streams for these
families go through every encoder branch they are named after. Every comparison is byte-exact.
Edge families through rio_encode_file (each record alone, then all in one shuffled batch), the launch
shapes at which each grid-stride loop goes round again, rio_device_encode called directly on device
tensors (capacity, guard bytes, NULL flags, a caller's stream, unaligned arenas, refusals), and the
tuning knobs in child processes."""
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import encode_cases as E
from encode_child import encode_file_arrays, first_difference
from recordio import _lib as L

pytestmark = pytest.mark.gpu

FAMILY_NAMES = [f.name for f in E.cached_families()]
PAD = L.RIO_DEVICE_PAD
GUARD = 64
FILL = 0xA5

_oracle = {}


def oracle(key, arrays, comp):
    """The oracle's (image, offsets) of a named batch, computed once and left unchanged."""
    if (key, comp) not in _oracle:
        img, off = E.oracle_arrays(*arrays, comp)
        img.setflags(write=False)
        off.setflags(write=False)
        _oracle[key, comp] = img, off
    return _oracle[key, comp]


def assert_file(got, arrays, comp, key, parse=True):
    """got = (status, out, offsets, length) of rio_encode_file / device_encode vs the oracle."""
    rc, out, roff, ln = got
    assert rc == 0, L.strerror(rc)
    want, want_off = oracle(key, arrays, comp)
    assert first_difference(out[:ln], want) is None, (key, comp, first_difference(out[:ln], want))
    assert np.array_equal(roff, want_off), (key, comp)
    if parse and comp == 2:
        for nil, u, c, pay in E.payloads(out[:ln].tobytes(), roff):
            assert len(pay) == (0 if nil else c)
            if not nil:
                assert sum(e[1] for e in E.elements(pay)) == u


# ---- edge families ------------------------------------------------------------------------------
@pytest.mark.parametrize("comp", [0, 2])
@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_family_each_record_alone(name, comp):
    f = next(f for f in E.cached_families() if f.name == name)
    for i, r in enumerate(f.records):
        arrays = E.to_arrays([r])
        assert_file(encode_file_arrays(*arrays, comp), arrays, comp, (name, i))


@pytest.mark.parametrize("comp", [0, 2])
def test_families_in_one_shuffled_batch(comp):
    arrays = E.to_arrays([r for _, _, r in E.shuffled_all()])
    assert_file(encode_file_arrays(*arrays, comp), arrays, comp, "families")


@pytest.mark.parametrize("comp", [0, 2])
def test_nil_record_with_a_span(comp):
    arrays, same_as = E.nil_span_batch()
    got = encode_file_arrays(*arrays, comp)
    assert_file(got, arrays, comp, "nil_span")
    assert_file(got, E.to_arrays(same_as), comp, "nil_span_list")


# ---- launch shapes: every grid-stride loop goes round a second time ---------------------------
def test_launch_global_table_slot_reuse():
    """8257 records over 1 KiB (k_snappy_encode_global: 8192 lanes), 70000-byte records at 10, 8202
    (the same lane and table slot, the same bytes) and 8229 (a slot that held a 2048-entry table)."""
    arrays = E.launch_global_reuse()
    assert_file(encode_file_arrays(*arrays, 2), arrays, 2, "global_reuse", parse=False)


def test_launch_lds_second_pass():
    """262161 small records: k_snappy_encode_lds<16,4> (16384 groups x 16) and k_enc_emit (65536
    lane groups) loop."""
    arrays = E.launch_lds_second_pass()
    assert_file(encode_file_arrays(*arrays, 2), arrays, 2, "lds_second_pass", parse=False)


@pytest.mark.parametrize("comp", [0, 2])
def test_launch_million_tiny(comp):
    """1048876 records of 0..3 bytes, some nil: the i <= n loops of k_enc_bounds / k_enc_sizes
    (1048576 threads) and the scans at that length."""
    arrays = E.launch_million_tiny()
    assert_file(encode_file_arrays(*arrays, comp), arrays, comp, "million_tiny", parse=False)


# ---- rio_device_encode on device tensors ---------------------------------------------------------
def device_encode(arrays, comp, cap=None, shift=0, null_flags=False, stream=None, ctx=None):
    """rio_device_encode: (status, d_out incl. GUARD bytes [host copy], offsets, *d_out_len). The
    arena starts `shift` bytes into its allocation and has PAD readable bytes after it; d_out is
    pre-filled with FILL; cap None = rio_encode_bound."""
    blob, off, flags = arrays
    n, total = int(off.shape[0]) - 1, int(off[-1])
    dev = torch.device("cuda:0")
    arena = torch.zeros(shift + total + PAD, dtype=torch.uint8, device=dev)
    if total:
        arena[shift:shift + total] = torch.from_numpy(np.array(blob[:total])).to(dev)
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    d_flags = torch.from_numpy(np.concatenate([flags, np.zeros(1, np.uint8)])).to(dev)
    cap = int(L.lib().rio_encode_bound(n, total, comp)) if cap is None else cap
    d_out = torch.full((cap + GUARD,), FILL, dtype=torch.uint8, device=dev)
    d_roff = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
    d_len = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    rc = L.lib().rio_device_encode(ctx or L.default_ctx(0), arena.data_ptr() + shift, d_off.data_ptr(),
                                   None if null_flags else d_flags.data_ptr(), n, total, comp, d_out.data_ptr(), cap,
                                   d_roff.data_ptr(), d_len.data_ptr(), stream.cuda_stream if stream else None)
    if stream:
        stream.synchronize()
    torch.cuda.synchronize()
    return rc, d_out.cpu().numpy(), d_roff.cpu().numpy().view(np.uint64)[:n], int(d_len.item())


@functools.lru_cache(maxsize=None)
def small_batch():
    """A batch with both encode kernels, several blocks, nil and empty records (about 400 KB)."""
    recs = [E.text(n, 20 + n % 7) for n in (1, 16, 17, 300, 1024, 1025, 5000, 65536, 70000)]
    recs += [None, b"", bytes(150000), E.rnd(random.Random(3), 3000), None]
    recs += E.cached_families()[0].records[::9]
    return E.to_arrays(recs)


@pytest.mark.parametrize("comp", [0, 2])
def test_direct_exact_capacity_and_guard_bytes(comp):
    arrays = small_batch()
    want, _ = oracle("small", arrays, comp)
    got = device_encode(arrays, comp, cap=len(want))
    assert_file(got, arrays, comp, "small")
    assert got[3] == len(want)
    assert np.all(got[1][len(want):] == FILL) and got[1][len(want):].shape[0] == GUARD


@pytest.mark.parametrize("comp", [0, 2])
def test_direct_bound_capacity_touches_nothing_past_the_file(comp):
    arrays = small_batch()
    got = device_encode(arrays, comp)
    assert_file(got, arrays, comp, "small")
    assert np.all(got[1][got[3]:] == FILL)


@pytest.mark.parametrize("comp", [0, 2])
def test_one_byte_short_writes_nothing(comp):
    arrays = small_batch()
    want, _ = oracle("small", arrays, comp)
    rc, out, _, ln = device_encode(arrays, comp, cap=len(want) - 1)
    assert rc == 0 and ln == len(want)  # stream-ordered: the caller reads the shortfall from *d_out_len
    assert np.all(out == FILL)
    rc, out, _, ln = encode_file_arrays(*arrays, comp, out_cap=len(want) - 1, fill=FILL)
    assert rc == L.RIO_ERR_CAPACITY and ln == len(want)
    assert np.all(out == FILL)


@pytest.mark.parametrize("comp", [0, 2])
def test_null_flags_equal_zero_flags(comp):
    blob, off, flags = small_batch()
    arrays = (blob, off, np.zeros_like(flags))  # nil records become empty ones
    a = device_encode(arrays, comp, null_flags=True)
    assert_file(a, arrays, comp, "small_no_nil")
    b = device_encode(arrays, comp)
    assert a[3] == b[3] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("comp", [0, 2])
def test_caller_stream(comp):
    arrays = small_batch()
    assert_file(device_encode(arrays, comp, stream=torch.cuda.Stream()), arrays, comp, "small")


@pytest.mark.parametrize("comp", [0, 2])
@pytest.mark.parametrize("shift", [1, 3, 7])
def test_unaligned_arena(shift, comp):
    arrays = small_batch()
    assert_file(device_encode(arrays, comp, shift=shift), arrays, comp, "small")


@pytest.mark.parametrize("comp", [0, 2])
def test_encode_file_offsets_relative_to_a_nonzero_first_record(comp):
    blob, off, flags = small_batch()
    moved = (np.concatenate([np.full(37, 0xEE, np.uint8), blob]), off + np.uint64(37), flags)
    got = encode_file_arrays(*moved, comp)
    assert_file(got, (blob, off, flags), comp, "small")


def test_history_independence():
    """One context: large records, then many tiny ones, then the large ones again (the scratch, the
    hash tables and the header slots are reused)."""
    big = E.to_arrays([E.text(70000, 30), bytes(150000), E.text(131072 + 40, 31), E.text(16385, 32)])
    rng = np.random.default_rng(8)
    tiny = E.to_arrays([bytes(rng.integers(0x61, 0x64, int(k), dtype=np.uint8)) for k in rng.integers(0, 40, 5000)])
    first = device_encode(big, 2)
    assert_file(first, big, 2, "history_big")
    assert_file(device_encode(tiny, 2), tiny, 2, "history_tiny")
    third = device_encode(big, 2)
    assert first[3] == third[3] and np.array_equal(first[1], third[1]) and np.array_equal(first[2], third[2])


def test_refusals():
    lib, ctx = L.lib(), L.default_ctx(0)
    dev = torch.device("cuda:0")
    rec = torch.zeros(16 + PAD, dtype=torch.uint8, device=dev)
    off = torch.tensor([0, 16], dtype=torch.int64, device=dev)
    out = torch.full((256,), FILL, dtype=torch.uint8, device=dev)
    roff = torch.zeros(1, dtype=torch.int64, device=dev)
    ln = torch.zeros(1, dtype=torch.int64, device=dev)
    good = [ctx, rec.data_ptr(), off.data_ptr(), None, 1, 16, 2, out.data_ptr(), 256, roff.data_ptr(), ln.data_ptr(), None]
    for null in (0, 2, 7, 10, 1):  # ctx, d_rec_off, d_out, d_out_len; d_records with n > 0
        args = list(good)
        args[null] = None
        assert lib.rio_device_encode(*args) == L.RIO_ERR_ARG, null
    for comp in (1, 3):
        args = list(good)
        args[6] = comp
        assert lib.rio_device_encode(*args) == L.RIO_ERR_UNSUPPORTED, comp
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and int(ln.item()) == 0
    assert lib.rio_device_encode(*good) == 0  # and the same arguments untouched are accepted
    torch.cuda.synchronize()
    want, _ = E.oracle_arrays(np.zeros(16, np.uint8), np.array([0, 16], np.uint64), np.zeros(1, np.uint8), 2)
    assert out.cpu().numpy()[:int(ln.item())].tobytes() == want.tobytes()


@pytest.mark.parametrize("comp", [0, 2])
def test_no_records_is_the_file_header(comp):
    empty = (np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint8))
    rc, out, roff, ln = device_encode(empty, comp, cap=8)
    assert rc == 0 and ln == 8 and roff.shape[0] == 0
    assert out[:8].tobytes() == bytes([4, 0, 0, 0, comp, 0, 0, 0]) and np.all(out[8:] == FILL)
    # d_records and d_out_rec_off may be NULL when there is nothing to encode
    dev = torch.device("cuda:0")
    off = torch.zeros(1, dtype=torch.int64, device=dev)
    d_out = torch.full((8 + GUARD,), FILL, dtype=torch.uint8, device=dev)
    d_len = torch.zeros(1, dtype=torch.int64, device=dev)
    rc = L.lib().rio_device_encode(L.default_ctx(0), None, off.data_ptr(), None, 0, 0, comp, d_out.data_ptr(), 8, None,
                                   d_len.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and int(d_len.item()) == 8 and np.array_equal(d_out.cpu().numpy(), out)


# ---- tuning knobs: read once per process, so one fresh child per value ---------------------------
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "encode_child.py")
CHILD_TIMEOUT = 120  # seconds; a child takes a few
_child_died = []


@pytest.mark.parametrize("knob,value", [("RIO_ENC_LANES", "64"), ("RIO_ENC_LANES", "32"), ("RIO_ENC_LANES", "8"),
                                        ("RIO_ENC_LDS", "0"), ("RIO_ENC_GROUPS", "1")])
def test_tuning_knob(knob, value):
    """One child at a time, no retry, and none after a child that ended by signal or timeout."""
    assert not _child_died, f"not started: {_child_died[0]}"
    env = {k: v for k, v in os.environ.items() if not k.startswith("RIO_ENC_")}
    env[knob] = value
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [CHILD]
    try:
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _child_died.append(f"{knob}={value} ran into its {CHILD_TIMEOUT} s limit")
        raise
    last = (p.stdout.strip().splitlines() or [""])[-1]
    if p.returncode < 0:
        _child_died.append(f"{knob}={value} ended by signal {-p.returncode}")
    assert p.returncode == 0, (p.returncode, last)
    assert last == f"ok [{knob}={value}]", last
