// The library's counter-based random stream, shared by the units that draw on the device (propose.hip: the sampler's tree
// proposals; domain.hip: candidates of the acquisition search).  Philox4x32-10; word pairs (0,1) and (2,3) of a block are one
// 64-bit draw x each (low word first), u = (x >> 11) * 2^-53.  Each unit documents its own key and counter layout.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bark {

__device__ __forceinline__ void philox(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1, c3 = (uint32_t)p0, c0 = n0, c2 = n2;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}
__device__ __forceinline__ double uniform53(uint32_t lo, uint32_t hi) {
    return (double)((((uint64_t)hi << 32) | lo) >> 11) * 0x1p-53;
}
// floor(u n) in 0 .. n - 1 (u n can round up to n)
__device__ __forceinline__ int64_t pick(double u, int64_t n) {
    const int64_t k = (int64_t)(u * (double)n);
    return k < n ? k : n - 1;
}

}  // namespace bark
