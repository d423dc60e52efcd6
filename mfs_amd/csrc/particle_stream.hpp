// particle_stream.hpp -- what the particle filters of every state dimension share on the device (particle_kernel.hpp: d = 1,
// particle_nd_kernel.hpp: d = 2): the Philox4x32-10 stream with its conversions (include/mfs_hip.h states them), the block
// sums in a fixed order, the block scan of the weights, the ancestor search of the resamplers and the component pick of the
// initial mixture.  Every sum and every draw that the filters' "same bits alone or in a batch" rests on is written here, once.
// __device__ helpers only, no kernels, so any translation unit may include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfs_hip.h"   // MFS_RESAMPLE_*
#include "registry.hpp"          // kPfThreads, kPfItems, kPfChunk

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

// ---------------------------------------------------------------------------------------------------------------
// the block scan of the weights.  Thread tid owns the particles i0 + 0 .. kPfItems - 1 (i0 = blk kPfChunk + tid kPfItems) and
// brings their running sums pre[j] and their total `run`.  Block-local inclusive prefix sums -> ws[i0 + j] (i0 + j < n), block
// total -> *block_total.  Every thread of the block calls it; `wave_tot` holds kPfThreads / 64 doubles of LDS.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pf_weight_scan(const double (&pre)[kPfItems], const double run, const int i0, const int n,
                                               double* ws, double* block_total, double* wave_tot) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // inclusive scan of the thread totals inside the wave, then the exclusive offset of this thread
    double inc = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    double exc = __shfl_up(inc, 1, 64);
    if (lane == 0) exc = 0.0;
    if (lane == 63) wave_tot[wv] = inc;
    __syncthreads();
    double base = 0.0, total = 0.0;
#pragma unroll
    for (int q = 0; q < kPfThreads / 64; ++q) {
        if (q == wv) base = total;
        total += wave_tot[q];
    }
    base += exc;
#pragma unroll
    for (int j = 0; j < kPfItems; ++j)
        if (i0 + j < n) ws[i0 + j] = base + pre[j];
    if (tid == 0) *block_total = total;
}

// ---------------------------------------------------------------------------------------------------------------
// resampling (tag 2): the uniform that systematic resampling shares among the particles of a step (0 for stratified, which
// draws one per particle), and the ancestor of particle i
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double pf_systematic_uniform(const int resampling, const uint64_t seed, const int t) {
    if (resampling != MFS_RESAMPLE_SYSTEMATIC) return 0.0;
    const PfWords r = pf_words(seed, 0, t, 2, 0);
    return pf_uniform(r.r0, r.r1);
}

// target v_i = (i + u_i) / n tot; the ancestor is the first j with cs[j] = offs[j / kPfChunk] + ws[j] >= v_i, side left
__device__ __forceinline__ int pf_ancestor(const int resampling, const uint64_t seed, const int t, const int i, const int n,
                                           const double u_sys, const double tot, const double* offs, const double* ws) {
    double u = u_sys;
    if (resampling != MFS_RESAMPLE_SYSTEMATIC) {
        const PfWords r = pf_words(seed, i, t, 2, 0);
        u = pf_uniform(r.r0, r.r1);
    }
    const double target = ((double)i + u) / (double)n * tot;
    // the first j in [0, n) with cs[j] >= target, n if there is none; every probe is inside [0, n - 1], and a comparison
    // with NaN sends the search right, so the result is clamped whatever the sums hold
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        const double c = offs[mid / kPfChunk] + ws[mid];
        if (c >= target) hi = mid; else lo = mid + 1;
    }
    return (lo < n - 1) ? lo : n - 1;
}

// the component of the initial mixture that the uniform uc picks: the number of cumulative weights <= uc, at most n_mix - 1
__device__ __forceinline__ int pf_mixture_pick(const double* mix_cumw,const int n_mix, const double uc) {
    int c = 0;
    for (int k = 0; k < n_mix; ++k) c += (mix_cumw[k] <= uc) ? 1 : 0;
    return (c < n_mix - 1) ? c : n_mix - 1;
}

}  // namespace mfs
