"""MMapReader.ReadNextAt / SeekNext with no decoded index behind them (GPU).

A reader whose file decodes to more than RIO_READAT_INDEX_MAX bytes (4 GiB unless set) builds no index:
every call runs the single-record kernels (k_read_at / k_seek_next, csrc/rio_seek.hip), and for gzip /
lzw the host expands the located record as a file of its own (readat_expand, csrc/rio_reader.cpp). With
an index in place those paths only ever see offsets that are not record starts. The variable is read
once per process, so tests/readat_child.py runs in a fresh process per value: it asserts n_records == 0
through rio_reader_index_info first, then compares both calls with the oracle at every record start and
at seeded offsets:

  RIO_READAT_INDEX_MAX=0      every record form of tests/snappy_streams.py behind k_read_at's one-thread
                              Snappy decoder, the `ends` Snappy file, and records of 2^20 - 1, 2^20,
                              2^20 + 1 and 3 * 2^20 bytes, Snappy and uncompressed, which take
                              read_at_impl's output buffer past its first 1 MiB (grow and retry)
  RIO_READAT_INDEX_MAX=65536  gzip and lzw files of 4 to 16 KiB records (a nil, a corrupt, an empty and a
                              two-member one among them) through readat_expand, and one 70 000-byte
                              record that it refuses with RIO_ERR_CAPACITY, as the same cap bounds it
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "readat_child.py")
# seconds; a child takes a few. The limit is there for a child that hangs, as in tests/test_gpu_encode_edges.py:
# nothing is started after one that ran into it or ended by signal, so a faulted device is not used again
CHILD_TIMEOUT = 120
_child_died = []


@pytest.mark.parametrize("cap,files", [("0", 4), ("65536", 2)])
def test_kernel_only_reader_equals_the_oracle(cap, files):
    """One child at a time, no retry, and none after a child that ended by signal or timeout."""
    assert not _child_died, f"not started: {_child_died[0]}"
    env = dict(os.environ, RIO_READAT_INDEX_MAX=cap)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [CHILD]
    try:
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _child_died.append(f"RIO_READAT_INDEX_MAX={cap} ran into its {CHILD_TIMEOUT} s limit")
        raise
    last = (p.stdout.strip().splitlines() or [""])[-1]
    if p.returncode < 0:
        _child_died.append(f"RIO_READAT_INDEX_MAX={cap} ended by signal {-p.returncode}")
    assert p.returncode == 0, (p.returncode, last)
    assert last == f"ok [RIO_READAT_INDEX_MAX={cap}] {files} files", last
