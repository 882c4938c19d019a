// rio_scan.hip — the one scan of the segmented copies: lengths (or flags) of n items plus a closing zero become
// n + 1 offsets, the last one the total. Every plan that sizes an output by a length pass calls this, so hipcub's
// scan kernels are instantiated here alone.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "rio_launch.h"

namespace rio {

size_t scan_cub_bytes(uint64_t n) {
    size_t b = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)(n + 1)) != hipSuccess)
        return 0;
    return b;
}

hipError_t launch_offsets_scan(void* cub_tmp, size_t cub_bytes, const uint64_t* in, uint64_t* out, uint64_t n,
                               hipStream_t s) {
    return hipcub::DeviceScan::ExclusiveSum(cub_tmp, cub_bytes, in, out, (int)(n + 1), s);
}

}  // namespace rio
