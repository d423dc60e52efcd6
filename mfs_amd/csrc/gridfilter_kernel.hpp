// gridfilter_kernel.hpp -- hand-written HIP for gfx950 (MI355X): the brute-force grid filter, i.e. the Chapman--Kolmogorov
// filter of mfs/classical_filters_smoothers/brute_force.py:26-136 on a spatial grid shared by B replicates.
//
//   build     K[i][j] = w_j N(x_i; m_j, s_j): the transition density from grid point j to grid point i times the trapezoid
//             weight of j, so that one sub-step of the prediction (brute_force.py:83-86, 114-120) is p <- K p
//   gemm      C = A B in fp64 on the matrix core (v_mfma_f64_16x16x4_f64).  The same kernel squares K (n x n x n, the power
//             route: K^S once, by binary exponentiation) and propagates the batch (P <- M P, n x n x B, P stored [n][B])
//   update    per replicate column: l_i = p(y | x_i) P[i][b], z = sum_i w_i l_i, P[i][b] = l_i / z, nell_b -= log z, and the
//             posterior mean and central variance as trapezoid integrals (brute_force.py:133)
//   cf        on request, the characteristic function of every posterior at given frequencies: a table of weighted cosines
//             and sines, one more product with the same GEMM per measurement, and a store (at the end of this file)
//
// Every matrix lives in a library-owned buffer padded with zeros to a multiple of kGridTile in both dimensions, so the GEMM
// has no edge branches and no out-of-range access for any n or B; padded rows and columns stay zero under every product.
// All reductions have a fixed order (one wave per output tile walks k in ascending order; the column sums of the update are
// summed per thread in a fixed stride and then in lane order): two runs give the same bits.  No atomics.
// The kernels are not templates: this header belongs to one translation unit (gridfilter_inst.hip); what capi.hip needs of
// it -- tile constants, GridUpdateArgs, the launchers -- is in registry.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfs_hip.h"
#include "likelihood.hpp"   // likelihood(); device_util.hpp: finite()
#include "registry.hpp"     // kGridTile, kGridBK; GridUpdateArgs (kernel_args.hpp)

namespace mfs {

// ---------------------------------------------------------------------------------------------------------------
// K and the initial densities
// ---------------------------------------------------------------------------------------------------------------
// grid (n_pad / 64, n_pad), 64 threads: row i = blockIdx.y, column j.  Entries outside n x n are zero.
__global__ void __launch_bounds__(64) grid_build_k(const int n, const int n_pad, const double* __restrict__ xs,
                                                   const double* __restrict__ m, const double* __restrict__ sd,
                                                   const double* __restrict__ w, double* __restrict__ K) {
    const int i = blockIdx.y, j = blockIdx.x * 64 + threadIdx.x;
    double v = 0.0;
    if (i < n && j < n) {
        const double s = sd[j], z = (xs[i] - m[j]) / s;
        v = exp(-0.5 * z * z) / (2.50662827463100050242 * s) * w[j];
    }
    K[(size_t)i * n_pad + j] = v;
}

// grid (ldp / 64, n_pad), 64 threads: P[i][b] = init[b][i] (or init[i]); zero outside n x B.
__global__ void __launch_bounds__(64) grid_init_p(const int n, const int B, const int ldp, const double* __restrict__ init,
                                                  const int init_batched, double* __restrict__ P) {
    const int i = blockIdx.y, b = blockIdx.x * 64 + threadIdx.x;
    double v = 0.0;
    if (i < n && b < B) v = init[(init_batched ? (size_t)b * n : 0) + i];
    P[(size_t)i * ldp + b] = v;
}

// ---------------------------------------------------------------------------------------------------------------
// C[M][N] = A[M][Kd] B[Kd][N], row-major, M and N multiples of 64, Kd a multiple of 16; C must not alias A or B.
// One 256-thread block per 64 x 64 tile of C; wave w owns the 32 x 32 quadrant (w >> 1, w & 1) as 2 x 2 MFMA tiles of 16 x 16
// (4 accumulators = 32 registers).  A and B slices of 16 k go through LDS, two buffers, one barrier per slice: the next slice is
// loaded into registers before the MFMAs of the current one and stored after them.  Operand map of v_mfma_f64_16x16x4_f64:
// A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15], D[(lane >> 4) + 4 r][lane & 15] in register r.
// LDS rows are padded so that the 32 lanes of one ds_read_b64 group hit 32 distinct 8-byte banks: A rows of 18 doubles
// (lanes: 16 rows x 2 k -> 18 i + k mod 32 all distinct), B rows of 80 (2 k x 16 columns -> 80 k + j = 16 k + j mod 32).
// ---------------------------------------------------------------------------------------------------------------
constexpr int kGridLdA = kGridBK + 2, kGridLdB = kGridTile + 16;
constexpr int kGridStage = kGridTile * kGridLdA + kGridBK * kGridLdB;   // doubles per LDS buffer

typedef double grid_d4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) grid_gemm(const double* __restrict__ A, const size_t lda, const double* __restrict__ Bm,
                                                 const size_t ldb, double* __restrict__ C, const size_t ldc, const int Kd) {
    __shared__ __attribute__((aligned(16))) double smem[2 * kGridStage];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv >> 1, wn = wv & 1, r16 = lane & 15, kk = lane >> 4;
    const size_t row0 = (size_t)blockIdx.y * kGridTile, col0 = (size_t)blockIdx.x * kGridTile;
    // staging: A slice 64 x 16, thread -> (row tid / 4, 4 doubles at k = 4 (tid % 4)); B slice 16 x 64 -> (k tid / 16, 4 columns)
    const int a_r = tid >> 2, a_k = (tid & 3) * 4, b_k = tid >> 4, b_c = (tid & 15) * 4;
    const double* ag = A + (row0 + a_r) * lda + a_k;
    const double* bg = Bm + (size_t)b_k * ldb + col0 + b_c;
    const int a_s = a_r * kGridLdA + a_k, b_s = kGridTile * kGridLdA + b_k * kGridLdB + b_c;

    grid_d4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = grid_d4{0.0, 0.0, 0.0, 0.0};

    double2 ra0 = *reinterpret_cast<const double2*>(ag), ra1 = *reinterpret_cast<const double2*>(ag + 2);
    double2 rb0 = *reinterpret_cast<const double2*>(bg), rb1 = *reinterpret_cast<const double2*>(bg + 2);
    *reinterpret_cast<double2*>(smem + a_s) = ra0; *reinterpret_cast<double2*>(smem + a_s + 2) = ra1;
    *reinterpret_cast<double2*>(smem + b_s) = rb0; *reinterpret_cast<double2*>(smem + b_s + 2) = rb1;
    __syncthreads();

    const int nk = Kd / kGridBK;
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;
        if (more) {
            const double* an = ag + (size_t)(kt + 1) * kGridBK;
            const double* bn = bg + (size_t)(kt + 1) * kGridBK * ldb;
            ra0 = *reinterpret_cast<const double2*>(an); ra1 = *reinterpret_cast<const double2*>(an + 2);
            rb0 = *reinterpret_cast<const double2*>(bn); rb1 = *reinterpret_cast<const double2*>(bn + 2);
        }
        const double* As = smem + cur * kGridStage + (32 * wm + r16) * kGridLdA + kk;
        const double* Bs = smem + cur * kGridStage + kGridTile * kGridLdA + kk * kGridLdB + 32 * wn + r16;
#pragma unroll
        for (int k4 = 0; k4 < kGridBK / 4; ++k4) {
            const double a0 = As[4 * k4], a1 = As[16 * kGridLdA + 4 * k4];
            const double b0 = Bs[4 * k4 * kGridLdB], b1 = Bs[4 * k4 * kGridLdB + 16];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (more) {
            double* nx = smem + (cur ^ 1) * kGridStage;
            *reinterpret_cast<double2*>(nx + a_s) = ra0; *reinterpret_cast<double2*>(nx + a_s + 2) = ra1;
            *reinterpret_cast<double2*>(nx + b_s) = rb0; *reinterpret_cast<double2*>(nx + b_s + 2) = rb1;
        }
        __syncthreads();
        cur ^= 1;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                C[(row0 + 32 * wm + 16 * i + kk + 4 * r) * ldc + col0 + 32 * wn + 16 * j + r16] = acc[i][j][r];
}

// ---------------------------------------------------------------------------------------------------------------
// Measurement update of step a.t.  256 threads = 8 replicate columns x 32 row lanes (column fastest, so a row's 8 columns are
// one 64-byte segment); grid = ceil(B / 8).  Row lane r walks i = r, r + 32, ... in each of the three passes, so every entry of
// a column is read and written by one thread only and the passes need no ordering beyond the block-wide sums.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kGridCols = 8, kGridRows = 32;

// the column's total of the 32 row-lane partials, in lane order; every thread of the block calls it
__device__ __forceinline__ double grid_col_sum(const double v, double* __restrict__ red, const int c, const int r) {
    __syncthreads();
    red[c * (kGridRows + 1) + r] = v;
    __syncthreads();
    double s = 0.0;
    for (int q = 0; q < kGridRows; ++q) s += red[c * (kGridRows + 1) + q];
    return s;
}

__global__ void __launch_bounds__(256) grid_update(const GridUpdateArgs a) {
    __shared__ double red[kGridCols * (kGridRows + 1)];
    const int c = threadIdx.x & (kGridCols - 1), r = threadIdx.x >> 3;
    const int b = blockIdx.x * kGridCols + c;
    const bool act = b < a.B;
    const int n = act ? a.n : 0;               // a column past B has nothing to do but joins the barriers
    double lp[MFS_MAX_LIK];
#pragma unroll
    for (int k = 0; k < MFS_MAX_LIK; ++k)
        lp[k] = (act && k < a.n_lik) ? a.lik[(a.lik_batched ? (size_t)b * a.n_lik : 0) + k] : 0.0;
    const double y = act ? a.ys[(size_t)b * a.T + a.t] : 0.0;
    double* Pc = a.P + b;
    const size_t ld = (size_t)a.ldp;

    // l_i = p(y | x_i) p_pred(x_i), z = int l
    double part = 0.0;
    for (int i = r; i < n; i += kGridRows) {
        const double l = likelihood(a.lik_kind, lp, y, a.xs[i]) * Pc[i * ld];
        Pc[i * ld] = l;
        part += a.w[i] * l;
    }
    const double z = grid_col_sum(part, red, c, r);
    const bool ok = (z > 0.0) && finite(z);
    const double qnan = __builtin_nan("");

    // posterior l / z (NaN from here on if the normaliser is zero or not finite) and its mean
    double* out = a.out_pdfs ? a.out_pdfs + ((size_t)b * a.T + a.t) * a.n : nullptr;
    part = 0.0;
    for (int i = r; i < n; i += kGridRows) {
        const double p = ok ? Pc[i * ld] / z : qnan;
        Pc[i * ld] = p;
        if (out) out[i] = p;
        part += a.w[i] * a.xs[i] * p;
    }
    const double mean = grid_col_sum(part, red, c, r);

    part = 0.0;
    for (int i = r; i < n; i += kGridRows) {
        const double d = a.xs[i] - mean;
        part += a.w[i] * d * d * Pc[i * ld];
    }
    const double var = grid_col_sum(part, red, c, r);

    if (act && r == 0) {
        a.out_means[(size_t)b * a.T + a.t] = mean;
        a.out_vars[(size_t)b * a.T + a.t] = var;
        a.nell[b] = ok ? a.nell[b] - log(z) : qnan;
        if (!ok && a.first_nan[b] < 0) a.first_nan[b] = a.t;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Characteristic function of a density on the grid, cf(z_k) = sum_i w_i exp(i z_k x_i) p_i
// (characteristic_from_pdf, mfs/one_dim/moments.py:340-343, as post_processing_brute_force.py:27-50 takes it of every
// posterior), as a product with a table of trapezoid-weighted cosines and sines:
//
//   table     E[k][i] = w_i cos(z_k x_i), E[m_pad + k][i] = w_i sin(z_k x_i): fp64 sincos of the rounded product z_k x_i at
//             every entry (no rotation recurrence, so `zs` needs no spacing), zero outside m x n.  Built once per call
//   gemm      grid_gemm as it is: C[2 m_pad][ldp] = E[2 m_pad][n_pad] P[n_pad][ldp] after the update of a step (the filter),
//             or C[rows][2 m_pad] = Ps[rows][n_pad] E^T[n_pad][2 m_pad] for densities stored by rows (mfs_cf_from_pdf_1d: the
//             table is written transposed, the densities are not)
//   store     (re, im) pairs out of the two halves of C, 16 bytes per thread, a row of frequencies contiguous
//
// m_pad = grid_pad(nz), n_pad = grid_pad(n), ldp = grid_pad(B).  Device working set of the filter's cf: the table,
// 2 m_pad n_pad doubles (256 MB at n = nz = 4096, 1 GB at the limits 8192 x 8192, the order of the power route's three n x n
// buffers); one product buffer, 2 m_pad ldp doubles (33 MB at nz = 2000, B = 1000); and two output blocks of S steps each,
// B S nz pairs, with S chosen so that a block stays within 64 MB (one step if a step is larger): while one block travels to
// the host the next S steps fill the other, whatever T is.
// The table is finite, so a NaN of P stays in its own column (row) of the product; the filter's store writes NaN for a
// poisoned replicate explicitly all the same.
// ---------------------------------------------------------------------------------------------------------------
// grid (cols / 64, rows), 64 threads.  transposed = 0: row k < m_pad, column i < n_pad, E[k][i] and E[m_pad + k][i] with
// ld = n_pad.  transposed = 1: row i < n_pad, column k < m_pad, E^T[i][k] and E^T[i][m_pad + k] with ld = 2 m_pad.
__global__ void __launch_bounds__(64) grid_cf_table(const int n, const int nz, const int n_pad, const int m_pad,
                                                    const int transposed, const double* __restrict__ xs,
                                                    const double* __restrict__ w, const double* __restrict__ zs,
                                                    double* __restrict__ E) {
    const int slow = blockIdx.y, fast = blockIdx.x * 64 + threadIdx.x;
    const int k = transposed ? fast : slow, i = transposed ? slow : fast;
    double c = 0.0, s = 0.0;
    if (k < nz && i < n) {
        const double arg = zs[k] * xs[i];
        sincos(arg, &s, &c);
        c *= w[i];
        s *= w[i];
    }
    if (transposed) {
        E[(size_t)i * (2 * (size_t)m_pad) + k] = c;
        E[(size_t)i * (2 * (size_t)m_pad) + m_pad + k] = s;
    } else {
        E[(size_t)k * n_pad + i] = c;
        E[((size_t)m_pad + k) * n_pad + i] = s;
    }
}

// The filter's store: out[b][slot][k] = (C[k][b], C[m_pad + k][b]), out being a block of [B][S][nz] pairs and `slot` the step's
// place in it; NaN in both parts if the replicate is poisoned (first_nan[b] >= 0: the update of this step has run).
// grid (ldp / 32, m_pad / 32), 256 threads: a 32 x 32 tile of each half goes through LDS, read with b fastest (256-byte
// segments of C), written with k fastest (512-byte segments of out).
constexpr int kGridCfTile = 32;

__global__ void __launch_bounds__(256) grid_cf_store(const int nz, const int B, const int m_pad, const int ldp, const int S,
                                                     const int slot, const double* __restrict__ Cm,
                                                     const int32_t* __restrict__ first_nan, double2* __restrict__ out) {
    __shared__ double re[kGridCfTile][kGridCfTile + 1], im[kGridCfTile][kGridCfTile + 1];
    const int k0 = blockIdx.y * kGridCfTile, b0 = blockIdx.x * kGridCfTile;
    const int f = threadIdx.x & (kGridCfTile - 1), q = threadIdx.x >> 5;
#pragma unroll
    for (int j = 0; j < kGridCfTile / 8; ++j) {
        const int kk = q + 8 * j;                      // C rows k0 + kk < m_pad, columns b0 + f < ldp: inside the padded buffer
        re[kk][f] = Cm[(size_t)(k0 + kk) * ldp + b0 + f];
        im[kk][f] = Cm[((size_t)m_pad + k0 + kk) * ldp + b0 + f];
    }
    __syncthreads();
    const double qnan = __builtin_nan("");
#pragma unroll
    for (int j = 0; j < kGridCfTile / 8; ++j) {
        const int bb = q + 8 * j, b = b0 + bb, k = k0 + f;
        if (b < B && k < nz) {
            const bool bad = first_nan[b] >= 0;
            out[((size_t)b * S + slot) * nz + k] = bad ? double2{qnan, qnan} : double2{re[f][bb], im[f][bb]};
        }
    }
}

// The store of densities by rows: out[c][k] = (C[c][k], C[c][m_pad + k]) for c < rows, k < nz.  grid (m_pad / 64, rows), 64 threads.
__global__ void __launch_bounds__(64) grid_cf_store_rows(const int nz, const int m_pad, const double* __restrict__ Cm,
                                                         double2* __restrict__ out) {
    const int c = blockIdx.y, k = blockIdx.x * 64 + threadIdx.x;
    if (k < nz) {
        const double* row = Cm + (size_t)c * (2 * (size_t)m_pad);
        out[(size_t)c * nz + k] = double2{row[k], row[m_pad + k]};
    }
}

}  // namespace mfs
