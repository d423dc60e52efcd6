// particle_stream.hpp -- what the particle filters of every state dimension share on the device (particle_kernel.hpp: d = 1,
// particle_nd_kernel.hpp: d = 2): the Philox4x32-10 stream with its conversions (include/mfs_hip.h states them) and the block
// sums in a fixed order.  __device__ helpers only, no kernels, so any translation unit may include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "registry.hpp"          // kPfThreads

namespace mfs {

// ---------------------------------------------------------------------------------------------------------------
// the stream
// ---------------------------------------------------------------------------------------------------------------
struct PfWords { uint32_t r0, r1, r2, r3; };

__device__ __forceinline__ PfWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return PfWords{c0, c1, c2, c3};
}

__device__ __forceinline__ PfWords pf_words(const uint64_t seed, const int i, const int t, const int tag, const int draw) {
    return philox4x32_10((uint32_t)i, (uint32_t)t, (uint32_t)tag, (uint32_t)draw, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// 52 bits + 1/2 on the 2^-52 lattice: exact, strictly inside (0, 1)
__device__ __forceinline__ double pf_uniform(const uint32_t a, const uint32_t b) {
    return ((double)(a >> 6) * 67108864.0 + (double)(b >> 6) + 0.5) * 2.220446049250313080847e-16;
}

__device__ __forceinline__ double pf_normal(const PfWords r) {
    return sqrt(-2.0 * log(pf_uniform(r.r0, r.r1))) * cos(6.283185307179586476925 * pf_uniform(r.r2, r.r3));
}

// ---------------------------------------------------------------------------------------------------------------
// block sums in a fixed order: butterfly inside each wave, then the four wave totals in index order.  Every thread of the
// block calls it; `red` holds kPfThreads / 64 doubles.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double pf_block_sum(double v, double* __restrict__ red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int q = 1; q < kPfThreads / 64; ++q) s += red[q];
    return s;
}

// the block totals of one replicate, added in index order (what `offsets` and `finalize` do for their outputs too)
__device__ __forceinline__ double pf_ordered_sum(const double* __restrict__ part, const int count) {
    double acc = 0.0;
    for (int k = 0; k < count; ++k) acc += part[k];
    return acc;
}

}  // namespace mfs
