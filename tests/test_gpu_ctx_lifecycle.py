"""Context lifecycle (GPU): destroying a context returns its device memory.

Twelve times over: rio_ctx_create, one pass through every feature that keeps scratch arenas in the context
(encode + decode, memstore flush with a bloom filter, merge-compaction of two views, WAL ops plan + gather, an
index search large enough for the query sort), rio_ctx_destroy. The inputs are built once on the device from a
seed and everything torch allocates is allocated on one stream, so torch's footprint is constant from the second
cycle on and the device's free memory after cycle 12 must be what it was after cycle 2.

Bound: with n = 2^18 every 8-byte-per-item arena is 2 MiB; one such arena leaked per cycle costs 20 MiB over the
ten cycles between the two readings, and the bound is half of that, 10 MiB.
Measured on MI355X before the arenas owned their memory (destroy freed them from a hand-kept list): drift 0 bytes.
"""
import ctypes

import pytest
import torch

import memstore as MS
from recordio import _lib as L
from sstables import bloom
from sstables.merger import compact_on_device

pytestmark = pytest.mark.gpu

N = 1 << 18
CYCLES, FIRST_READ = 12, 2
BOUND = 10 << 20
SEED = 20261020
_NONE = 0xFFFFFFFFFFFFFFFF
INFO_BYTES = ctypes.sizeof(L.FileInfo)
HIT_BYTES = ctypes.sizeof(L.IndexHit)


class Inputs:
    """N keys (ascending, 8 bytes big-endian) and N random 8-byte values, and what each feature takes of them."""

    def __init__(self, dev):
        g = torch.Generator(device=dev)
        g.manual_seed(SEED)
        i64 = lambda *a, **k: torch.arange(*a, dtype=torch.int64, device=dev, **k)  # noqa: E731
        pad = torch.zeros(L.RIO_DEVICE_PAD, dtype=torch.uint8, device=dev)
        k = 2 * i64(N) + torch.randint(0, 2, (N,), device=dev, generator=g)  # strictly ascending
        shifts = i64(56, -8, -8)
        be = lambda x: ((x.unsqueeze(1) >> shifts) & 255).to(torch.uint8)  # noqa: E731
        self.key_rows = be(k)
        self.val_rows = torch.randint(0, 256, (N, 8), dtype=torch.uint8, device=dev, generator=g)
        self.keys = torch.cat([self.key_rows.reshape(-1), pad])
        self.values = torch.cat([self.val_rows.reshape(-1), pad])
        self.off8 = 8 * i64(N + 1)
        self.zeros8 = torch.zeros(N + L.RIO_DEVICE_PAD, dtype=torch.uint8, device=dev)
        # memstore flush: the same pairs as an op log in a random order
        perm = torch.randperm(N, device=dev, generator=g)
        self.op_keys = torch.cat([self.key_rows[perm].reshape(-1), pad])
        self.op_values = torch.cat([self.val_rows[perm].reshape(-1), pad])
        self.ops = L.OpsView(keys=self.op_keys.data_ptr(), key_off=self.off8.data_ptr(), values=self.op_values.data_ptr(),
                             val_off=self.off8.data_ptr(), flags=self.zeros8.data_ptr(), n=N, key_bytes=8 * N,
                             value_bytes=8 * N)
        # merge: the even and the odd entries as two loaded tables
        h = N // 2
        self.tables = []
        for t in range(2):
            tk = torch.cat([self.key_rows[t::2].reshape(-1), pad])
            tv = torch.cat([self.val_rows[t::2].reshape(-1), pad])
            self.tables.append((tk, tv))
        self.key_len = torch.full((h,), 8, dtype=torch.int64, device=dev)
        self.crc = torch.randint(0, 1 << 62, (h,), dtype=torch.int64, device=dev, generator=g)
        self.views = (L.SstView * 2)(*[
            L.SstView(index=tk.data_ptr(), key_off=self.off8.data_ptr(), key_len=self.key_len.data_ptr(), data=tv.data_ptr(),
                      data_off=self.off8.data_ptr(), flags=self.zeros8.data_ptr(), crc=self.crc.data_ptr(), n=h,
                      index_bytes=8 * h, data_bytes=8 * h) for tk, tv in self.tables])
        # WAL: WalMutation{addition{key = 3: bytes, value = 4: bytes}} per pair, 22 bytes each
        rec = torch.empty((N, 22), dtype=torch.uint8, device=dev)
        rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = 0x0A, 20, 0x1A, 8
        rec[:, 4:12] = self.key_rows
        rec[:, 12], rec[:, 13] = 0x22, 8
        rec[:, 14:22] = self.val_rows
        self.wal = torch.cat([rec.reshape(-1), pad])
        self.wal_off = 22 * i64(N + 1)
        self.segs = (L.WalSegment * 1)(L.WalSegment(out=self.wal.data_ptr(), out_off=self.wal_off.data_ptr(),
                                                    flags=self.zeros8.data_ptr(), n=N, out_bytes=22 * N))
        self.filter_keys = [int(x) for x in torch.randint(0, 1 << 62, (4,), generator=torch.Generator().manual_seed(SEED))]
        torch.cuda.synchronize()


def cycle(inp, dev, st):
    """One context's life; every call must return RIO_OK. Runs with `st` as torch's current stream."""
    lib = L.lib()
    sp = ctypes.c_void_p(st.cuda_stream)
    i64 = lambda n: torch.empty(n, dtype=torch.int64, device=dev)  # noqa: E731
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)  # noqa: E731
    h = ctypes.c_void_p()
    assert lib.rio_ctx_create(0, ctypes.byref(h)) == L.RIO_OK
    ctx = h.value

    # encode N records, decode the image: the records come back
    cap = int(lib.rio_encode_bound(N, 8 * N, L.COMP_SNAPPY))
    img, img_off, img_len = torch.zeros(cap + L.RIO_DEVICE_PAD, dtype=torch.uint8, device=dev), i64(N), i64(1)
    assert lib.rio_device_encode(ctx, inp.values.data_ptr(), inp.off8.data_ptr(), None, N, 8 * N, L.COMP_SNAPPY,
                                 img.data_ptr(), cap, img_off.data_ptr(), img_len.data_ptr(), sp) == L.RIO_OK
    flen = int(img_len.item())
    out, out_off, rec_off, flags = u8(8 * N + 16), i64(N + 1), i64(N), u8(N)
    info = torch.zeros(INFO_BYTES, dtype=torch.uint8, device=dev)
    assert lib.rio_device_decode(ctx, img.data_ptr(), flen, out.data_ptr(), out.numel(), out_off.data_ptr(),
                                 rec_off.data_ptr(), flags.data_ptr(), N, info.data_ptr(), sp) == L.RIO_OK
    fi = L.FileInfo.from_buffer_copy(info.cpu().numpy().tobytes())
    assert fi.status == L.RIO_EOF and fi.n_records == N and fi.total_out_bytes == 8 * N and fi.n_bad == 0
    assert torch.equal(out[:8 * N], inp.values[:8 * N]) and torch.equal(out_off, inp.off8)
    assert torch.equal(rec_off, img_off) and not bool(flags.any())

    # memstore flush with a bloom filter: plan, gather, bloom add, both encodes, index entries
    c = MS.flush_ops_on_device(ctx, 0, inp.ops, L.RIO_FLUSH_WITH_TOMBSTONES, L.COMP_SNAPPY, max_key_len=8,
                               flt=bloom.Filter(8 * N, inp.filter_keys))
    assert c.status is None and c.n_out == N and c.first_dup == _NONE and c.bloom is not None

    # merge-compaction of two views
    c = compact_on_device(ctx, 0, inp.views, L.RIO_MERGE_LATEST_WINS, L.COMP_NONE)
    assert c.status is None and c.n_out == N and c.first_dup == _NONE

    # WAL ops of one segment
    res = i64(L.RIO_WAL_RESULT_WORDS)
    assert lib.rio_wal_ops_plan(ctx, ctypes.addressof(inp.segs), 1, res.data_ptr(), sp) == L.RIO_OK
    r = [x & _NONE for x in res.cpu().tolist()]
    assert r[L.RIO_WAL_R_FIRST_BAD] == _NONE
    assert (r[L.RIO_WAL_R_N_RECORDS], r[L.RIO_WAL_R_N_OPS], r[L.RIO_WAL_R_KEY_BYTES], r[L.RIO_WAL_R_VALUE_BYTES]) == \
        (N, N, 8 * N, 8 * N)
    wk, wv, wko, wvo, wf, wr = u8(8 * N), u8(8 * N), i64(N + 1), i64(N + 1), u8(N), i64(N)
    assert lib.rio_wal_ops_gather(ctx, N, wk.data_ptr(), 8 * N, wko.data_ptr(), wv.data_ptr(), 8 * N, wvo.data_ptr(),
                                  wf.data_ptr(), wr.data_ptr(), sp) == L.RIO_OK

    # index search of every key in the merged table's index.rio: N >= 4096 queries take the query sort
    hits = u8(N * HIT_BYTES)
    assert lib.rio_device_index_search(ctx, c.index_img.data_ptr(), int(c.index_len.item()), 0, inp.keys.data_ptr(),
                                       inp.off8.data_ptr(), N, hits.data_ptr(), sp) == L.RIO_OK
    hv = hits.view(torch.int32).reshape(N, HIT_BYTES // 4)
    assert int(hv[:, 6].abs().sum()) == 0 and int(hv[:, 7].sum()) == N  # status, found

    st.synchronize()
    lib.rio_ctx_destroy(ctx)


def test_destroyed_contexts_return_their_memory():
    dev = "cuda:0"
    L.lib()
    inp = Inputs(dev)
    st = torch.cuda.Stream(device=dev)
    free = {}
    with torch.cuda.device(0), torch.cuda.stream(st):
        for i in range(1, CYCLES + 1):
            cycle(inp, dev, st)
            if i in (FIRST_READ, CYCLES):
                torch.cuda.synchronize(0)
                free[i] = torch.cuda.mem_get_info(0)[0]
    drift = free[FIRST_READ] - free[CYCLES]
    print(f"free after cycle {FIRST_READ}: {free[FIRST_READ]}, after cycle {CYCLES}: {free[CYCLES]}, drift {drift} bytes")
    assert drift < BOUND, drift
