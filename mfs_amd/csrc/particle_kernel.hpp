// particle_kernel.hpp -- hand-written HIP for gfx950 (MI355X): the bootstrap particle filter of
// mfs/classical_filters_smoothers/smc.py:26-84 with the stratified / systematic resamplers of resampling.py:43-59, for B
// replicates x n particles in fp64.  The particles live in HBM ([B][n]); a replicate spans pf_blocks(n) workgroups.
//
// One measurement t is five launches on one stream (PfArgs, kernel_args.hpp):
//   propagate  x_i <- mu(x_i) + sqrt(var(x_i)) z_i (the model tables of MFS_TRANS_GAUSSIAN), w_i = p(y_t | x_i), and the
//              block-local inclusive prefix sums of w: per thread over its kPfItems consecutive particles, then the block scan
//              (pf_weight_scan, particle_stream.hpp).  Block total -> wpart
//   offsets    one thread per replicate adds the block totals in index order: woffs (exclusive), wtot, nell -= log(wtot / n),
//              and the NaN rule: wtot zero or not finite -> first_nan, nell = NaN.  The kernel of every state dimension, with
//              an argument struct of its own (PfOffsetsArgs)
//   resample   x'_i = x[idx_i], idx_i the ancestor of particle i (pf_ancestor, particle_stream.hpp: target (i + u_i) / n wtot,
//              binary search over woffs[j / kPfChunk] + wscan[j], clamped to [0, n - 1]).  Block total of x' -> xpart
//   cf         per segment of kPfSeg particles: sum of (x' - mean)^2 and, for each frequency, of exp(i z_k x').  A thread owns F
//              consecutive frequencies and walks the segment's particles (staged in LDS) in index order; on a uniform z grid it
//              takes one true sincos per particle at its first frequency and rotates by exp(i dz x') for the other F - 1 <= 7
//   finalize   adds the block / segment totals in index order: out_means, out_vars, out_cfs
//
// The random stream is Philox4x32-10 with key = the replicate's seed and counter = (particle, step, tag, draw), so a draw does
// not depend on the launch geometry or on the batch (include/mfs_hip.h states the conversions).  No atomics: every sum runs in
// an order fixed by n and the constants of registry.hpp, so two runs, and a replicate alone or in a batch, give the same bits.
// The kernels of one translation unit (particle_inst.hip); what capi.hip needs is in registry.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfs_hip.h"
#include "likelihood.hpp"        // likelihood(); device_util.hpp: horner(), finite()
#include "particle_stream.hpp"   // the stream, the ordered sums, pf_weight_scan, pf_ancestor, pf_mixture_pick
#include "registry.hpp"          // kPf*; PfArgs, PfOffsetsArgs (kernel_args.hpp)

namespace mfs {

// (the stream, the sums, the weight scan and the ancestor search, shared with the d = 2 filter: particle_stream.hpp)
__global__ void __launch_bounds__(kPfThreads) pf_draws(const uint64_t seed, const int t, const int tag, const int draw,
                                                       const int count, double* __restrict__ out_u, double* __restrict__ out_z) {
    const int i = blockIdx.x * kPfThreads + threadIdx.x;
    if (i >= count) return;
    const PfWords r = pf_words(seed, i, t, tag, draw);
    out_u[i] = pf_uniform(r.r0, r.r1);
    out_z[i] = pf_normal(r);
}

// ---------------------------------------------------------------------------------------------------------------
// initial particles (tag 0, t = 0).  grid (nblk, B)
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPfThreads) pf_init(const PfArgs a) {
    const int b = blockIdx.y;
    const uint64_t seed = a.seeds[b];
    double* x = a.x + (size_t)b * a.n;
#pragma unroll
    for (int j = 0; j < kPfItems; ++j) {
        const int i = blockIdx.x * kPfChunk + j * kPfThreads + threadIdx.x;
        if (i >= a.n) continue;
        if (a.n_mix > 0) {
            const double z = pf_normal(pf_words(seed, i, 0, 0, 0));
            const PfWords r = pf_words(seed, i, 0, 0, 1);
            const int c = pf_mixture_pick(a.mix_cumw, a.n_mix, pf_uniform(r.r0, r.r1));
            x[i] = a.mix_mean[c] + sqrt(a.mix_var[c]) * z;
        } else {
            x[i] = a.init[(a.init_batched ? (size_t)b * a.n : 0) + i];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// propagate, weight, block scan.  grid (nblk, B); thread tid owns the particles blk kPfChunk + tid kPfItems + 0 .. kPfItems - 1
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPfThreads) pf_propagate(const PfArgs a) {
    __shared__ double wave_tot[kPfThreads / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    const uint64_t seed = a.seeds[b];
    const int J1 = a.degree + 1;
    const double* coef = a.coef + (a.coef_batched ? (size_t)b * 2 * J1 : 0);
    double lp[MFS_MAX_LIK];
#pragma unroll
    for (int k = 0; k < MFS_MAX_LIK; ++k) lp[k] = (k < a.n_lik) ? a.lik[(a.lik_batched ? (size_t)b * a.n_lik : 0) + k] : 0.0;
    const double y = a.ys[(size_t)b * a.T + a.t];
    double* x = a.x + (size_t)b * a.n;
    double* ws = a.wscan + (size_t)b * a.n;
    const int i0 = blockIdx.x * kPfChunk + tid * kPfItems;
    const double qnan = __builtin_nan("");

    double pre[kPfItems], run = 0.0;
#pragma unroll
    for (int j = 0; j < kPfItems; ++j) {
        const int i = i0 + j;
        double w = 0.0;                 // a particle past n weighs nothing
        if (i < a.n) {
            const double xv = x[i];
            const double u = (a.umap == MFS_U_TANH) ? tanh(xv) : xv;
            const double mu = a.mean_x_coef * xv + horner(coef, a.degree, u);
            const double var = horner(coef + J1, a.degree, u);
            const double z = pf_normal(pf_words(seed, i, a.t, 1, 0));
            const double xn = (var > 0.0 && finite(var)) ? mu + sqrt(var) * z : qnan;
            x[i] = xn;
            w = likelihood(a.lik_kind, lp, y, xn);
        }
        run += w;
        pre[j] = run;
    }
    pf_weight_scan(pre, run, i0, a.n, ws, a.wpart + (size_t)b * a.nblk + blockIdx.x, wave_tot);
}

// ---------------------------------------------------------------------------------------------------------------
// block offsets, sum of the weights, NLL and the NaN rule.  One thread per replicate; grid ceil(B / 64), 64 threads
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) pf_offsets(const PfOffsetsArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const double* part = a.wpart + (size_t)b * a.nblk;
    double* offs = a.woffs + (size_t)b * a.nblk;
    double acc = 0.0;
    for (int k = 0; k < a.nblk; ++k) {
        offs[k] = acc;
        acc += part[k];
    }
    a.wtot[b] = acc;
    const bool ok = (acc > 0.0) && finite(acc);
    a.nell[b] = ok ? a.nell[b] - log(acc / (double)a.n) : __builtin_nan("");
    if (!ok && a.first_nan[b] < 0) a.first_nan[b] = a.t;
}

// ---------------------------------------------------------------------------------------------------------------
// resample.  grid (nblk, B); thread tid owns the particles blk kPfChunk + tid + q kPfThreads (coalesced)
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPfThreads) pf_resample(const PfArgs a) {
    __shared__ double red[kPfThreads / 64];
    const int b = blockIdx.y, n = a.n;
    const uint64_t seed = a.seeds[b];
    const double* x = a.x + (size_t)b * n;
    const double* ws = a.wscan + (size_t)b * n;
    const double* offs = a.woffs + (size_t)b * a.nblk;
    double* x2 = a.x2 + (size_t)b * n;
    double* out = a.out_samples ? a.out_samples + ((size_t)b * a.T + a.t) * n : nullptr;
    const double tot = a.wtot[b];
    const bool ok = (tot > 0.0) && finite(tot);
    const double u_sys = pf_systematic_uniform(a.resampling, seed, a.t);
    double part = 0.0;
#pragma unroll
    for (int q = 0; q < kPfItems; ++q) {
        const int i = blockIdx.x * kPfChunk + q * kPfThreads + threadIdx.x;
        if (i >= n) continue;
        const int idx = pf_ancestor(a.resampling, seed, a.t, i, n, u_sys, tot, offs, ws);
        const double xn = ok ? x[idx] : __builtin_nan("");
        x2[i] = xn;
        if (out) out[i] = xn;
        part += xn;
    }
    const double total = pf_block_sum(part, red);
    if (threadIdx.x == 0) a.xpart[(size_t)b * a.nblk + blockIdx.x] = total;
}

// ---------------------------------------------------------------------------------------------------------------
// variance and characteristic function of the resampled particles.  grid (nseg, B, frequency chunks of kPfThreads F)
// ---------------------------------------------------------------------------------------------------------------
template <int F>
__global__ void __launch_bounds__(kPfThreads) pf_cf(const PfArgs a) {
    __shared__ double sx[kPfChunk], sc[kPfChunk], ss[kPfChunk];
    __shared__ double red[kPfThreads / 64];
    __shared__ double s_mean;
    const int b = blockIdx.y, seg = blockIdx.x, tid = threadIdx.x, n = a.n, nz = a.nz;
    const bool first = blockIdx.z == 0;             // the frequency chunk that also sums the variance
    const bool rotate = F > 1 && a.z_uniform != 0;
    const double* x2 = a.x2 + (size_t)b * n;
    if (tid == 0) s_mean = pf_ordered_sum(a.xpart + (size_t)b * a.nblk, a.nblk) / (double)n;
    const int k0 = (blockIdx.z * kPfThreads + tid) * F;
    double zf[F], re[F], im[F];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        zf[f] = (k0 + f < nz) ? a.zs[k0 + f] : 0.0;
        re[f] = 0.0;
        im[f] = 0.0;
    }
    double vacc = 0.0;
    for (int base = seg * kPfSeg; base < n && base < (seg + 1) * kPfSeg; base += kPfChunk) {
        __syncthreads();                            // the previous chunk has been read (first pass: s_mean is written)
#pragma unroll
        for (int q = 0; q < kPfItems; ++q) {
            const int p = q * kPfThreads + tid, i = base + p;
            const double xv = (i < n) ? x2[i] : 0.0;
            sx[p] = xv;
            if (rotate) {
                double s, c;
                sincos(a.dz * xv, &s, &c);
                sc[p] = c;
                ss[p] = s;
            }
        }
        __syncthreads();
        const int cnt = (n - base < kPfChunk) ? n - base : kPfChunk;
        if (first) {
            const double mean = s_mean;
#pragma unroll
            for (int q = 0; q < kPfItems; ++q) {
                const int p = q * kPfThreads + tid;
                if (p < cnt) {
                    const double d = sx[p] - mean;
                    vacc += d * d;
                }
            }
        }
        if (k0 < nz) {
            for (int p = 0; p < cnt; ++p) {
                const double xv = sx[p];
                if (rotate) {
                    double s, c;
                    sincos(zf[0] * xv, &s, &c);
                    re[0] += c;
                    im[0] += s;
                    const double cd = sc[p], sd = ss[p];
#pragma unroll
                    for (int f = 1; f < F; ++f) {
                        const double cn = c * cd - s * sd, sn = s * cd + c * sd;
                        c = cn;
                        s = sn;
                        re[f] += c;
                        im[f] += s;
                    }
                } else {
#pragma unroll
                    for (int f = 0; f < F; ++f) {
                        double s, c;
                        sincos(zf[f] * xv, &s, &c);
                        re[f] += c;
                        im[f] += s;
                    }
                }
            }
        }
    }
    if (a.cfpart) {
        double* out = a.cfpart + ((size_t)b * a.nseg + seg) * nz * 2;
#pragma unroll
        for (int f = 0; f < F; ++f)
            if (k0 + f < nz) {
                out[2 * (k0 + f)] = re[f];
                out[2 * (k0 + f) + 1] = im[f];
            }
    }
    if (first) {
        const double total = pf_block_sum(vacc, red);
        if (tid == 0) a.vpart[(size_t)b * a.nseg + seg] = total;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// the step's outputs from the block / segment totals, in index order.  grid (ceil((2 nz + 2) / kPfThreads), B): element 0 the
// mean, 1 the variance, 2 + q entry q of the replicate's [nz][2] cf row
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPfThreads) pf_finalize(const PfArgs a) {
    const int b = blockIdx.y, e = blockIdx.x * kPfThreads + threadIdx.x;
    const size_t bt = (size_t)b * a.T + a.t;
    const double n = (double)a.n;
    if (e == 0) {
        a.out_means[bt] = pf_ordered_sum(a.xpart + (size_t)b * a.nblk, a.nblk) / n;
    } else if (e == 1) {
        a.out_vars[bt] = pf_ordered_sum(a.vpart + (size_t)b * a.nseg, a.nseg) / n;
    } else if (e - 2 < 2 * a.nz) {
        const int q = e - 2;
        const double* part = a.cfpart + (size_t)b * a.nseg * a.nz * 2 + q;
        double acc = 0.0;
        for (int k = 0; k < a.nseg; ++k) acc += part[(size_t)k * a.nz * 2];
        a.out_cfs[bt * a.nz * 2 + q] = acc / n;
    }
}

}  // namespace mfs
