// Test-only (not part of the product): the look-back cell scan k_scan_single (arpeggia_amd/csrc/scan.inl) on a caller's array, without the
// engine around it.  tests/test_scan_unit_gpu.py builds this file into libscan_unit.so and compares with numpy.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "arp_internal.h"

namespace arp {
#define DEVFN __device__ __forceinline__
#include "scan.inl"
}  // namespace arp

// cells of one register-held tile of a block: the test puts its sizes around blocks x this
extern "C" uint32_t scan_unit_tile_cells() { return arp::kScanTileCells; }

// Runs the scan with `blocks` blocks (256 or 1024) on n cells.  in_words = n + pad_in words and out_words = n + 1 + pad_out words are copied to
// the device whole, sentinels included, and copied back whole; the published chunk totals are zeroed first, as the grid sizing does.
// Returns 0, or -1 on a HIP error.
extern "C" int scan_unit_run(uint32_t blocks, uint32_t n, uint32_t *in, uint64_t in_words, uint32_t *out, uint64_t out_words) {
    if ((blocks != arp::kScanSingleBlocks && blocks != arp::kScanBlocks) || in_words < n || out_words < (uint64_t)n + 1u) return -1;
    uint32_t *d_in = nullptr, *d_out = nullptr, *d_n = nullptr;
    unsigned long long *d_part = nullptr;
    int rc = -1;
    if (hipMalloc((void **)&d_in, (in_words + 4u) * 4u) == hipSuccess && hipMalloc((void **)&d_out, (out_words + 4u) * 4u) == hipSuccess &&
        hipMalloc((void **)&d_n, 4u) == hipSuccess && hipMalloc((void **)&d_part, arp::kScanBlocks * 8u) == hipSuccess &&
        hipMemcpy(d_in, in, in_words * 4u, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d_out, out, out_words * 4u, hipMemcpyHostToDevice) == hipSuccess &&
        hipMemcpy(d_n, &n, 4u, hipMemcpyHostToDevice) == hipSuccess && hipMemset(d_part, 0, arp::kScanBlocks * 8u) == hipSuccess) {
        hipLaunchKernelGGL(arp::k_scan_single, dim3(blocks), dim3(arp::kScanThreads), 0, nullptr, d_in, (const uint32_t *)d_n, d_part, d_out);
        if (hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(in, d_in, in_words * 4u, hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(out, d_out, out_words * 4u, hipMemcpyDeviceToHost) == hipSuccess)
            rc = 0;
    }
    (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_n); (void)hipFree(d_part);
    return rc;
}
