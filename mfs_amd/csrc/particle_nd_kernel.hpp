// particle_nd_kernel.hpp -- hand-written HIP for gfx950 (MI355X): the bootstrap particle filter of
// mfs/classical_filters_smoothers/smc.py:26-84 for a two-dimensional state, as dardel/prey_predator/pf.py runs it (Normal
// proposal N(mu(x), S(x)) with a per-particle Cholesky factor, stratified / systematic resampling), for B replicates x n
// particles in fp64.  The particles live in HBM as [B][2][n], component-major, so every pass over them is coalesced; a
// replicate spans pf_blocks(n) workgroups.
//
// One measurement t is five launches on one stream (PfNdArgs, kernel_args.hpp):
//   propagate  mu, S from the five polynomials of MFS_ND_TRANS_GAUSSIAN at (x_0, x_1) (the table, this replicate's if batched,
//              staged in LDS); L the closed-form lower Cholesky factor of S; x'_0 = mu_0 + l_00 z_0, x'_1 = mu_1 + l_10 z_0 +
//              l_11 z_1, both NaN if a pivot is negative or not finite; w_i = prod_f lik_f(y_t[ycol_f], x'_i[component_f]); and
//              the block-local inclusive prefix sums of w by the 1-D filter's scan (pf_weight_scan).  Block total -> wpart
//   offsets    pf_offsets (particle_kernel.hpp), launched by the host with its own PfOffsetsArgs: woffs, wtot, nell -=
//              log(wtot / n), the NaN rule
//   resample   the 1-D filter's ancestor search (pf_ancestor) and NaN handling; the one ancestor index gathers both components,
//              and writes out_samples[b][t][i][0..1] as one 16-byte store.  Block totals of x'_0, x'_1 -> xpart
//   cov        per segment of kPfSeg particles: sums of d_0 d_0, d_0 d_1, d_1 d_1 with d = x' - mean -> cpart
//   finalize   adds the block / segment totals in index order: out_means, out_covs (both off-diagonal entries)
//
// The stream, the weight scan, the ancestor search and the mixture pick are the 1-D filter's (particle_stream.hpp).  Counter = (particle, step, tag, draw): tag 0 draws 0, 1 the initial
// normals z_0, z_1 and draw 2 the component uniform; tag 1 draw k the propagation normal of component k; tag 2 draw 0 the
// resampling uniform.  No atomics: every sum runs in an order fixed by n and the constants of registry.hpp.
// The kernels of one translation unit (particle_nd_inst.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfs_hip.h"
#include "likelihood.hpp"           // likelihood(); device_util.hpp: finite(), gf_poly2(), gf_chol2()
#include "particle_stream.hpp"      // the stream, the ordered sums, pf_weight_scan, pf_ancestor, pf_mixture_pick
#include "registry.hpp"             // kPf*; PfNdArgs (kernel_args.hpp)

namespace mfs {

constexpr int kPfNdCoefMax = 5 * MFS_ND_MAX_EXTENT_HI * MFS_ND_MAX_EXTENT_HI;   // doubles of the five staged polynomials

// ---------------------------------------------------------------------------------------------------------------
// initial particles (tag 0, t = 0).  grid (nblk, B)
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPfThreads) pfnd_init(const PfNdArgs a) {
    const int b = blockIdx.y, n = a.n;
    const uint64_t seed = a.seeds[b];
    double* x0 = a.x + (size_t)b * 2 * n;
    double* x1 = x0 + n;
#pragma unroll
    for (int j = 0; j < kPfItems; ++j) {
        const int i = blockIdx.x * kPfChunk + j * kPfThreads + threadIdx.x;
        if (i >= n) continue;
        if (a.n_mix > 0) {
            const double z0 = pf_normal(pf_words(seed, i, 0, 0, 0));
            const double z1 = pf_normal(pf_words(seed, i, 0, 0, 1));
            const PfWords r = pf_words(seed, i, 0, 0, 2);
            const int c = pf_mixture_pick(a.mix_cumw, a.n_mix, pf_uniform(r.r0, r.r1));
            const double* L = a.mix_chol + 4 * c;
            x0[i] = a.mix_mean[2 * c] + L[0] * z0;
            x1[i] = a.mix_mean[2 * c + 1] + L[2] * z0 + L[3] * z1;
        } else {
            const double* src = a.init + ((a.init_batched ? (size_t)b * n : 0) + i) * 2;
            x0[i] = src[0];
            x1[i] = src[1];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// propagate, weight, block scan.  grid (nblk, B); thread tid owns the particles blk kPfChunk + tid kPfItems + 0 .. kPfItems - 1
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPfThreads) pfnd_propagate(const PfNdArgs a) {
    __shared__ double s_coef[kPfNdCoefMax];
    __shared__ double wave_tot[kPfThreads / 64];
    const int b = blockIdx.y, tid = threadIdx.x, n = a.n;
    const uint64_t seed = a.seeds[b];
    const int D = a.extent, DD = D * D;
    const double* coef = a.coef + (a.coef_batched ? (size_t)b * a.coef_stride : 0);
    for (int e = tid; e < 5 * DD; e += kPfThreads) s_coef[e] = coef[e];
    double lp[MFS_ND_MAX_FACTORS][MFS_MAX_LIK], y[MFS_ND_MAX_FACTORS];
#pragma unroll
    for (int f = 0; f < MFS_ND_MAX_FACTORS; ++f) {
        const bool live = f < a.n_factors;
        const double* src = a.lik + ((a.lik_batched ? (size_t)b * a.n_factors : 0) + (live ? f : 0)) * MFS_MAX_LIK;
#pragma unroll
        for (int k = 0; k < MFS_MAX_LIK; ++k) lp[f][k] = live ? src[k] : 0.0;
        y[f] = live ? a.ys[((size_t)b * a.T + a.t) * a.ny + a.fac_ycol[f]] : 0.0;
    }
    double* x0 = a.x + (size_t)b * 2 * n;
    double* x1 = x0 + n;
    double* ws = a.wscan + (size_t)b * n;
    const int i0 = blockIdx.x * kPfChunk + tid * kPfItems;
    const double qnan = __builtin_nan("");
    __syncthreads();

    double pre[kPfItems], run = 0.0;
#pragma unroll
    for (int j = 0; j < kPfItems; ++j) {
        const int i = i0 + j;
        double w = 0.0;                 // a particle past n weighs nothing
        if (i < n) {
            const double v0 = x0[i], v1 = x1[i];
            const double mu0 = gf_poly2(s_coef, D, v0, v1), mu1 = gf_poly2(s_coef + DD, D, v0, v1);
            const double s00 = gf_poly2(s_coef + 2 * DD, D, v0, v1), s01 = gf_poly2(s_coef + 3 * DD, D, v0, v1);
            const double s11 = gf_poly2(s_coef + 4 * DD, D, v0, v1);
            double l00, l10, l11;
            const bool ok = gf_chol2(s00, s01, s11, l00, l10, l11);
            const double z0 = pf_normal(pf_words(seed, i, a.t, 1, 0));
            const double z1 = pf_normal(pf_words(seed, i, a.t, 1, 1));
            const double n0 = ok ? mu0 + l00 * z0 : qnan;
            const double n1 = ok ? mu1 + l10 * z0 + l11 * z1 : qnan;
            x0[i] = n0;
            x1[i] = n1;
            w = 1.0;
#pragma unroll
            for (int f = 0; f < MFS_ND_MAX_FACTORS; ++f)
                if (f < a.n_factors) w *= likelihood(a.fac_kind[f], lp[f], y[f], a.fac_component[f] ? n1 : n0);
        }
        run += w;
        pre[j] = run;
    }
    pf_weight_scan(pre, run, i0, n, ws, a.wpart + (size_t)b * a.nblk + blockIdx.x, wave_tot);
}

// ---------------------------------------------------------------------------------------------------------------
// resample.  grid (nblk, B); thread tid owns the particles blk kPfChunk + tid + q kPfThreads (coalesced)
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPfThreads) pfnd_resample(const PfNdArgs a) {
    __shared__ double red[kPfThreads / 64];
    const int b = blockIdx.y, n = a.n;
    const uint64_t seed = a.seeds[b];
    const double* x0 = a.x + (size_t)b * 2 * n;
    const double* x1 = x0 + n;
    const double* ws = a.wscan + (size_t)b * n;
    const double* offs = a.woffs + (size_t)b * a.nblk;
    double* y0 = a.x2 + (size_t)b * 2 * n;
    double* y1 = y0 + n;
    double2* out = a.out_samples ? reinterpret_cast<double2*>(a.out_samples) + ((size_t)b * a.T + a.t) * n : nullptr;
    const double tot = a.wtot[b];
    const bool ok = (tot > 0.0) && finite(tot);
    const double u_sys = pf_systematic_uniform(a.resampling, seed, a.t);
    double part0 = 0.0, part1 = 0.0;
#pragma unroll
    for (int q = 0; q < kPfItems; ++q) {
        const int i = blockIdx.x * kPfChunk + q * kPfThreads + threadIdx.x;
        if (i >= n) continue;
        const int idx = pf_ancestor(a.resampling, seed, a.t, i, n, u_sys, tot, offs, ws);
        const double n0 = ok ? x0[idx] : __builtin_nan(""), n1 = ok ? x1[idx] : __builtin_nan("");
        y0[i] = n0;
        y1[i] = n1;
        if (out) out[i] = make_double2(n0, n1);
        part0 += n0;
        part1 += n1;
    }
    const double total0 = pf_block_sum(part0, red);
    const double total1 = pf_block_sum(part1, red);
    if (threadIdx.x == 0) {
        a.xpart[((size_t)b * 2 + 0) * a.nblk + blockIdx.x] = total0;
        a.xpart[((size_t)b * 2 + 1) * a.nblk + blockIdx.x] = total1;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// covariance partials of the resampled particles about their mean.  grid (nseg, B)
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPfThreads) pfnd_cov(const PfNdArgs a) {
    __shared__ double red[kPfThreads / 64];
    __shared__ double s_mean[2];
    const int b = blockIdx.y, seg = blockIdx.x, tid = threadIdx.x, n = a.n;
    const double* x0 = a.x2 + (size_t)b * 2 * n;
    const double* x1 = x0 + n;
    if (tid < 2) s_mean[tid] = pf_ordered_sum(a.xpart + ((size_t)b * 2 + tid) * a.nblk, a.nblk) / (double)n;
    __syncthreads();
    const double m0 = s_mean[0], m1 = s_mean[1];
    double c00 = 0.0, c01 = 0.0, c11 = 0.0;
    for (int base = seg * kPfSeg; base < n && base < (seg + 1) * kPfSeg; base += kPfChunk) {
#pragma unroll
        for (int q = 0; q < kPfItems; ++q) {
            const int i = base + q * kPfThreads + tid;
            if (i < n) {
                const double d0 = x0[i] - m0, d1 = x1[i] - m1;
                c00 += d0 * d0;
                c01 += d0 * d1;
                c11 += d1 * d1;
            }
        }
    }
    const double t00 = pf_block_sum(c00, red);
    const double t01 = pf_block_sum(c01, red);
    const double t11 = pf_block_sum(c11, red);
    if (tid == 0) {
        double* out = a.cpart + (size_t)b * 3 * a.nseg + seg;
        out[0] = t00;
        out[a.nseg] = t01;
        out[2 * a.nseg] = t11;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// the step's outputs from the block / segment totals, in index order.  grid B, 64 threads: lanes 0, 1 the means, 2..4 the
// covariance entries (0,0), (0,1) = (1,0), (1,1)
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) pfnd_finalize(const PfNdArgs a) {
    const int b = blockIdx.x, e = threadIdx.x;
    const size_t bt = (size_t)b * a.T + a.t;
    const double n = (double)a.n;
    if (e < 2) {
        a.out_means[bt * 2 + e] = pf_ordered_sum(a.xpart + ((size_t)b * 2 + e) * a.nblk, a.nblk) / n;
    } else if (e < 5) {
        const double c = pf_ordered_sum(a.cpart + ((size_t)b * 3 + (e - 2)) * a.nseg, a.nseg) / n;
        double* out = a.out_covs + bt * 4;
        if (e == 2) out[0] = c;
        else if (e == 4) out[3] = c;
        else { out[1] = c; out[2] = c; }
    }
}

}  // namespace mfs
