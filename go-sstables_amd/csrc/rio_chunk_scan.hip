// rio_chunk_scan.hip — the chunk-summary scan: the second launch of the decode pipeline (overview: rio_place.hip;
// DESIGN.md §4).
//   k_scan_blocks   256-chunk blocks: inclusive scan of key-point chunk summaries (stitches each
//                   chunk's speculative entry to its predecessor's exit; a mismatch => sequential
//                   repair walk); the last block runs the top level: record/byte prefix sums,
//                   terminal status (FileReader.ReadNext loop, file_reader.go:61-131).
// The gzip and lzw redo rounds run it again over the resized records.
#include <hip/hip_runtime.h>

#include "rio_device.h"
#include "rio_dev_util.h"
#include "rio_frame.h"
#include "rio_launch.h"
#include "rio_wave.h"

namespace rio {

// ------------------------------------------------------------------------------------------
// Key-point run composition. combine(A, B): A's byte range precedes B's.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ RunSum run_identity() {
    RunSum r;
    r.key = kNone;
    r.out = 0;
    r.cnt = 0;
    r.bytes = 0;
    r.ce = 0;
    r.term = 0;
    r.broken = 0;
    r.term_chunk = 0;
    return r;
}

__device__ __forceinline__ RunSum combine(const RunSum& A, const RunSum& B) {
    if (B.ce == 0) return A;
    if (A.ce == 0) return B;
    if (A.key == kNone) {  // A owns nothing for the inputs the composite can represent
        RunSum r = B;
        return r;
    }
    RunSum r = A;
    r.ce = B.ce;
    if (A.broken || A.term) return r;
    const uint64_t y = A.out;
    if (y >= B.ce) return r;  // B passed through
    if (B.key != kNone && y == B.key) {
        r.out = B.out;
        r.cnt = A.cnt + B.cnt;
        r.bytes = A.bytes + B.bytes;
        r.term = B.term;
        r.broken = B.broken;
        r.term_chunk = B.term_chunk;
        return r;
    }
    r.broken = 1;
    return r;
}

__device__ __forceinline__ RunSum chunk_run(const FrameParams& P, uint64_t c) {
    const ChunkSum s = P.chunks[c];
    RunSum r;
    r.key = s.entry;
    r.out = s.exit;
    r.cnt = s.count;
    r.bytes = s.bytes;
    r.ce = chunk_end(P, c);
    r.term = s.status != RIO_OK;
    r.broken = 0;
    r.term_chunk = c;
    return r;
}

__device__ void scan_top(const FrameParams& P, RunSum (*buf)[kScanBlock]);
__device__ void scan_finish(const FrameParams& P, const RunSum& total);

// Level 1: inclusive scan of 256 chunk runs per block in LDS (Hillis-Steele, 8 steps). The last
// block to finish (arrival ticket) runs level 2 over the block runs: one launch for the scan.
__global__ void __launch_bounds__(kScanBlock) k_scan_blocks(FrameParams P) {
    __shared__ RunSum buf[2][kScanBlock];
    __shared__ uint32_t last;
    const int t = threadIdx.x;
    const uint64_t c = (uint64_t)blockIdx.x * kScanBlock + t;
    const uint32_t pf = code_pf(kPfScan);
    if (P.state->hdr_status != RIO_OK) return;  // block-uniform
    if (P.redo && (!P.state->gz_redo || P.state->compression != P.redo)) return;  // another codec's redo round
    RunSum v = c < P.n_chunks ? chunk_run(P, c) : run_identity();
    int cur = 0;
    buf[cur][t] = v;
    __syncthreads();
#pragma unroll 1
    for (int d = 1; d < kScanBlock; d <<= 1) {
        RunSum x = buf[cur][t];
        if (t >= d) x = combine(buf[cur][t - d], x);
        buf[cur ^ 1][t] = x;
        cur ^= 1;
        __syncthreads();
    }
    if (c < P.n_chunks) P.chunk_excl[c] = t > 0 ? buf[cur][t - 1] : run_identity();
    if (t == kScanBlock - 1) P.block_runs[blockIdx.x] = buf[cur][t];
    // release this block's run, take a ticket; the last arriver acquires every block's run
    __syncthreads();
    if (t == 0) {
        __threadfence();
        last = atomicAdd(&P.state->scan_ticket, 1u) == gridDim.x - 1;
    }
    code_pf_done(pf);
    __syncthreads();
    if (!last) return;
    __threadfence();
    scan_top(P, buf);
}

// Sequential repair (slow path): walks the true chain chunk by chunk, re-walking any chunk whose
// speculative entry does not match. Runs on one thread; only for files whose speculation broke.
__device__ void slow_path(const FrameParams& P, uint32_t ver, uint32_t comp) {
    ScanState* st = P.state;
    uint64_t cur = RIO_FILE_HEADER_BYTES, base_idx = 0, base_bytes = 0, repairs = 0;
    bool term = false;
    uint64_t term_chunk = 0;
    for (uint64_t c = 0; c < P.n_chunks; c++) {
        ChunkPlace pl{base_idx, base_bytes, 0};
        if (!term && cur < chunk_end(P, c)) {
            if (P.chunks[c].entry != cur) {
                walk_chunk(P, c, cur, ver, comp);
                repairs++;
            }
            const ChunkSum s = P.chunks[c];
            pl.owned = s.count;
            base_idx += s.count;
            base_bytes += s.bytes;
            if (s.status != RIO_OK) {
                term = true;
                term_chunk = c;
            } else {
                cur = s.exit;
            }
        }
        P.place[c] = pl;
    }
    st->slow = 1;
    st->n_repairs = repairs;
    st->n_records = base_idx;
    st->total_bytes = base_bytes;
    if (term) {
        const ChunkSum s = P.chunks[term_chunk];
        st->status = s.status;
        st->status_offset = s.err_off;
        st->det0 = s.det0;
        st->det1 = s.det1;
    } else {
        st->status = RIO_EOF;
        st->status_offset = cur;
    }
}

// Level 2 (k_scan_blocks' last block): scans the block runs in tiles of kScanBlock with a carry,
// decides fast/slow path and the terminal status.
__device__ void scan_top(const FrameParams& P, RunSum (*buf)[kScanBlock]) {
    __shared__ RunSum carry_s;
    ScanState* st = P.state;
    const int t = threadIdx.x;
    if (P.n_chunks == 0) {
        if (t == 0) {
            st->status = RIO_EOF;
            st->status_offset = P.len;
        }
        return;  // (len == 8: the first ReadNext hits EOF)
    }
    if (P.n_blocks <= 64) {
        // one wave, no block barriers: entries 0..63 of the 256-wide Hillis-Steele below are exactly this 64-lane
        // one (its steps d >= 64 leave them alone), and its total is entry 63 (combine returns the other operand
        // of an identity unchanged): the same association, so the same RunSums (files up to 16384 chunks)
        if (t >= 64) return;
        buf[0][t] = t < P.n_blocks ? P.block_runs[t] : run_identity();
        wave_sync_lds();
        int cur = 0;
#pragma unroll 1
        for (int d = 1; d < 64; d <<= 1) {
            RunSum x = buf[cur][t];
            if (t >= d) x = combine(buf[cur][t - d], x);
            buf[cur ^ 1][t] = x;
            cur ^= 1;
            wave_sync_lds();
        }
        if ((uint64_t)t < P.n_blocks) P.block_excl[t] = combine(run_identity(), t > 0 ? buf[cur][t - 1] : run_identity());
        if (t != 0) return;
        const RunSum total = combine(run_identity(), buf[cur][63]);
        scan_finish(P, total);
        return;
    }
    if (t == 0) carry_s = run_identity();
    __syncthreads();
    for (uint64_t base = 0; base < P.n_blocks; base += kScanBlock) {
        const uint64_t b = base + t;
        RunSum v = b < P.n_blocks ? P.block_runs[b] : run_identity();
        int cur = 0;
        buf[cur][t] = v;
        __syncthreads();
#pragma unroll 1
        for (int d = 1; d < kScanBlock; d <<= 1) {
            RunSum x = buf[cur][t];
            if (t >= d) x = combine(buf[cur][t - d], x);
            buf[cur ^ 1][t] = x;
            cur ^= 1;
            __syncthreads();
        }
        const RunSum carry = carry_s;
        RunSum excl = combine(carry, t > 0 ? buf[cur][t - 1] : run_identity());
        if (b < P.n_blocks) P.block_excl[b] = excl;
        __syncthreads();
        if (t == kScanBlock - 1) carry_s = combine(carry, buf[cur][t]);
        __syncthreads();
    }
    const RunSum total = carry_s;
    if (t != 0) return;
    scan_finish(P, total);
}

// The file's state from the composed run of all chunks (one thread): the terminal status, the counts, or the
// sequential repair when a speculative entry did not chain.
__device__ void scan_finish(const FrameParams& P, const RunSum& total) {
    ScanState* st = P.state;
    const uint32_t ver = st->version, comp = st->compression;
    // total.key is chunk 0's forced entry (8): total describes the true chain unless broken.
    if (total.broken) {
        slow_path(P, ver, comp);
        if (st->status == RIO_ERR_MAGIC && st->version != RIO_VERSION1) st->zero_from = st->status_offset + st->det0;
        return;
    }
    st->n_records = total.cnt;
    st->total_bytes = total.bytes;
    if (total.term) {
        const ChunkSum s = P.chunks[total.term_chunk];
        st->status = s.status;
        st->status_offset = s.err_off;
        st->det0 = s.det0;
        st->det1 = s.det1;
    } else {
        st->status = RIO_EOF;  // chain ended exactly at the file end
        st->status_offset = total.out;
    }
    if (st->status == RIO_ERR_MAGIC && st->version != RIO_VERSION1) st->zero_from = st->status_offset + st->det0;
}

// stop: the scan stage's event (may be null; the redo rounds pass none)
void launch_chunk_scan(const FrameParams& P, hipStream_t s, hipEvent_t stop) {
    launch_ev(k_scan_blocks, dim3(blocks_for(P.n_chunks, kScanBlock)), dim3(kScanBlock), s, nullptr, stop, P);
}

}  // namespace rio
