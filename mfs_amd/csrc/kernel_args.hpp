// kernel_args.hpp -- every argument struct a launcher takes, the constants the host reads off the kernels, and the graded-lex
// helpers of the d = 3 layout that host and device share.  Host-and-device, no kernel code: registry.hpp includes it, and
// through registry.hpp capi.hip sees what it fills in; the kernel headers include it for the struct their kernel is passed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfs_hip.h"

namespace mfs {

// ---- 1-D: dense and fast paths
struct Filter1dArgs {
    int mode, T, B, stable;
    int extra;   // 1: the moment vectors carry 2N + 1 entries (dense path only; the order-2N moment is an output, never an input)
    int t_begin, t_end;
    // model
    int trans_kind, umap, n_terms, degree, n_rows, coef_batched, lik_kind, n_lik, lik_batched;
    double mean_x_coef;
    const double* coef;
    const double* lik;
    // inputs
    const double* m0;
    int m0_batched;
    const double* mean0;
    const double* scale0;
    const double* ys;
    // carry between chunks: [B][2N], [B], [B], [B], [B]
    double* c_mom;
    double* c_mean;
    double* c_scale;
    double* c_nell;
    int32_t* c_first_nan;
    double* c_lam;  // [B][2][G] nodes (in rule units) and weights of the posterior atoms, i.e. the next predict-half rule (fast
                    // path, chunked runs only)
    int recompute_rule;   // 1: the predict-half rule is recomputed from the posterior moments (MFS_PREDICT_RULE=recompute)
    // outputs (any may be null except out_nell)
    double* out_mom;
    double* out_mean;
    double* out_scale;
    double* out_nell;
    int32_t* out_first_nan;
};

struct Quad1dArgs {
    int B, stable;
    const double* ms;
    const double* mean;
    const double* scale;
    double* out_w;
    double* out_x;
};

struct Cf1dArgs {
    int count, nz;
    const double* ms;     // [count][2N]
    const double* mean;   // [count] or null
    const double* scale;  // [count] or null
    const double* zs;     // [nz]
    double* out;          // [count][nz][2]  (re, im)
};

// the model table of a 1-D filter in LDS: every operator row (+ the variance row) at the highest degree
constexpr int kCoefDoubles = (MFS_MAX_TERMS + 1) * (MFS_MAX_DEGREE + 1);

// specialised one-wave builds of the fast kernel (filter1d_fast.hpp, SPEC): tables of at most kSpecTop padded degrees (their
// launcher types and tables, like every other, are declared in registry.hpp)
constexpr int kSpecTop = 4;

// ---- 1-D gradient
struct Filter1dGradArgs {
    Filter1dArgs f;          // the plain filter's arguments (model tables, inputs; out_mom / out_mean unused)
    int n_par;               // P
    const double* dcoef;     // [P][n_rows][degree + 1] (or [B][P][...] when coef_batched): d coef / d theta_p
    const double* dlik;      // [P][n_lik] (or [B][P][n_lik]): d (likelihood parameters) / d theta_p
    double* out_grad;        // [B][P]: d nell / d theta_p
};

// ---- N-D, d = 2
struct FilterNdArgs {
    int mode, T, B, stable;
    int t_begin, t_end;       // the steps this launch takes (a chunk of [0, T)); the state crosses launches through `carry`
    double* carry;            // [B][NdTile::kCarry] (or null): the slots NdTile::cMean .. cV name the layout
    int n_terms_used, D;      // coefficient block extent per variable (degree + 1)
    int n_factors, ny;        // likelihood = prod_f lik(kind_f, params_f, y[ycol_f], x[comp_f]);  ys is [B][T][ny]
    int fac_kind[2], fac_comp[2], fac_ycol[2];
    int coef_batched, lik_batched;
    int force_eigen;          // 1: every update diagonalises K_k (the checked fallback of the Chebyshev evaluation, as the only route)
    int joint_grid;           // 1: a likelihood of both components is integrated over the Chebyshev grid instead of the eigen-nodes (A/B)
    int ext[32];              // per-block true extents (ea | eb << 8) of the coefficient blocks; 0 = empty block
    const double* coef;       // [rows][D][D] (or [B][...]), rows = terms + 2 with terms = 14 or 27 (see nd_terms): Q_kappa in the
                              // fixed kappa order of filternd_kernel.hpp (kKap0, kKap1; zeros where the model has no term), then the
                              // conditional variances of X'_0, X'_1 (scaled mode)
    const double* lik;        // [n_factors][4] (or [B][n_factors][4])
    const int32_t* inds;      // [3][s][s]
    const double* m0;         // [z] or [B][z]
    int m0_batched;
    const double* mean0;      // [2] or [B][2]
    const double* scale0;     // [2] or [B][2] (scaled mode)
    const double* ys;         // [B][T][ny]
    double* out_mom;          // [B][T][z]
    double* out_mean;         // [B][T][2]
    double* out_scale;        // [B][T][2] (scaled mode)
    double* out_nell;
    int32_t* out_first_nan;
};

// ---- N-D, d = 3
struct FilterNd3Args {
    int mode, T, B, stable;
    int trans_kind;           // MFS_ND_TRANS_*
    int D;                    // coefficient block extent per variable
    int ext[MFS_ND3_ROWS];    // true extents of each block: ea | eb << 8 | ec << 16 (0 = empty block)
    int n_factors, ny;
    int fac_kind[MFS_ND3_MAX_FACTORS], fac_comp[MFS_ND3_MAX_FACTORS], fac_ycol[MFS_ND3_MAX_FACTORS];
    int coef_batched, lik_batched;
    const double* coef;       // [MFS_ND3_ROWS][D][D][D] (or [B][...]): operator rows 0..33 Q_kappa, 34..36 variances; Gaussian rows 0..8
    const double* lik;        // [n_factors][MFS_MAX_LIK] (or [B][...])
    const int32_t* inds;      // [4][s][s]
    const double* m0;         // [z] or [B][z]
    int m0_batched;
    const double* mean0;      // [3] or [B][3]
    const double* scale0;     // [3] or [B][3]
    const double* ys;         // [B][T][ny]
    double* out_mom;          // [B][T][z] or null
    double* out_mean;         // [B][T][3] or null
    double* out_scale;        // [B][T][3] or null
    double* out_nell;         // [B]
    int32_t* out_first_nan;   // [B] or null
};

// joint likelihood factors (mfs_joint_nd3): a second kernel argument of the J = 1 instantiations only
struct FilterNd3Joint {
    int n, E, batched;
    int kind[MFS_ND3_MAX_JOINT], link[MFS_ND3_MAX_JOINT], ycol[MFS_ND3_MAX_JOINT];
    int ext[MFS_ND3_MAX_JOINT][2];   // true extents of p and q, packed as FilterNd3Args::ext
    const double* coef;              // [n][2][E][E][E] (or [B][...])
    const double* par;               // [n] (or [B][n]): Gaussian variance
};

// graded-lexicographic multi-indices in three variables (multi_indices.py:139-177): by total degree, each degree in ascending
// tuple order.  Position of (a, b, c), count of |n| <= deg, and the exponents of position i -- all usable at compile time.
__host__ __device__ constexpr int nd3_count(int deg) { return (deg + 1) * (deg + 2) * (deg + 3) / 6; }
__host__ __device__ constexpr int nd3_index(int a, int b, int c) {
    return nd3_count(a + b + c - 1) + a * (a + b + c + 1) - a * (a - 1) / 2 + b;
}
__host__ __device__ constexpr int nd3_exp(int i, int k) {
    int idx = 0;
    for (int d = 0; d < 64; ++d)
        for (int a = 0; a <= d; ++a)
            for (int b = 0; b <= d - a; ++b) {
                if (idx == i) return k == 0 ? a : k == 1 ? b : d - a - b;
                ++idx;
            }
    return -1;
}
__host__ __device__ constexpr int nd3_perm(int n, int k) {   // n! / (n - k)!
    int r = 1;
    for (int m = 0; m < k; ++m) r *= n - m;
    return r;
}
// operator row of kappa: its graded-lex position minus one (kappa = 0 is implicit) -- the order of mfs_amd._lib.ND3_KAPPAS
__host__ __device__ constexpr int nd3_kappa_row(int a, int b, int c) { return nd3_index(a, b, c) - 1; }
static_assert(nd3_count(4) - 1 == MFS_ND3_TERMS, "34 operator terms with 1 <= |kappa| <= 4");
static_assert(nd3_kappa_row(0, 0, 1) == 0 && nd3_kappa_row(1, 0, 0) == 2 && nd3_kappa_row(4, 0, 0) == MFS_ND3_TERMS - 1, "kappa order");

// ---- brute-force grid filter: the measurement update
struct GridUpdateArgs {
    int n, T, B, t;          // grid points, steps, replicates, the step this launch updates
    int ldp;                 // leading dimension of P (the padded B)
    int lik_kind, n_lik, lik_batched;
    const double* xs;        // [n]
    const double* w;         // [n] trapezoid weights
    const double* lik;       // [n_lik] or [B][n_lik]
    const double* ys;        // [B][T]
    double* P;               // [n_pad][ldp]: predicted densities in, posteriors out
    double* out_pdfs;        // [B][T][n] or null
    double* out_means;       // [B][T]
    double* out_vars;        // [B][T]
    double* nell;            // [B], accumulated over the steps
    int32_t* first_nan;      // [B], -1 until a step's normaliser is zero or not finite
};

// ---- bootstrap particle filter
struct PfArgs {
    int n, T, B, t;          // particles, steps, replicates, the step this launch works on
    int nblk, nseg;          // pf_blocks(n), pf_segments(n)
    int resampling;          // MFS_RESAMPLE_*
    int umap, degree, coef_batched, lik_kind, n_lik, lik_batched;
    double mean_x_coef;
    const double* coef;      // [2][degree + 1] or [B][2][degree + 1]: P_m, P_v of MFS_TRANS_GAUSSIAN
    const double* lik;       // [n_lik] or [B][n_lik]
    const double* ys;        // [B][T]
    const uint64_t* seeds;   // [B]
    int n_mix, init_batched; // initial law: a mixture of n_mix Normals drawn on the device, or (n_mix = 0) given samples
    const double* mix_cumw;  // [n_mix] each
    const double* mix_mean;
    const double* mix_var;
    const double* init;      // [n] or [B][n]
    int nz, z_uniform;       // frequencies of the cf; 1: zs is uniformly spaced with step dz
    double dz;
    const double* zs;        // [nz]
    double* x;               // [B][n] the particles: propagated in place, read by the resampler
    double* x2;              // [B][n] the resampled particles (the host swaps x and x2 after every step)
    double* wscan;           // [B][n] block-local inclusive prefix sums of the weights
    double* wpart;           // [B][nblk] block totals of the weights
    double* woffs;           // [B][nblk] their exclusive prefix sums in index order
    double* wtot;            // [B] sum of the weights
    double* xpart;           // [B][nblk] block totals of the resampled particles
    double* vpart;           // [B][nseg] segment totals of (x' - mean)^2
    double* cfpart;          // [B][nseg][nz][2] segment totals of exp(i z x'), or null
    double* out_samples;     // [B][T][n] or null
    double* out_means;       // [B][T]
    double* out_vars;        // [B][T]
    double* out_cfs;         // [B][T][nz][2] or null
};
// what the `offsets` kernel reads and writes: the same kernel for every state dimension
struct PfOffsetsArgs {
    int n, B, t, nblk;       // particles, replicates, the step this launch works on, pf_blocks(n)
    double* wpart;           // [B][nblk] block totals of the weights (read)
    double* woffs;           // [B][nblk] their exclusive prefix sums in index order
    double* wtot;            // [B] sum of the weights
    double* nell;            // [B], accumulated over the steps
    int32_t* first_nan;      // [B], -1 until a step's weight sum is zero or not finite
};

// ---- bootstrap particle filter, d = 2: the particles are [B][2][n], component-major, so every particle pass is coalesced
struct PfNdArgs {
    int n, T, B, t;          // particles, steps, replicates, the step this launch works on
    int nblk, nseg;          // pf_blocks(n), pf_segments(n)
    int resampling;          // MFS_RESAMPLE_*
    int extent, coef_stride, coef_batched;   // D; doubles between two replicates' tables (rows D D); 1: one table per replicate
    int n_factors, ny, lik_batched;
    int fac_kind[MFS_ND_MAX_FACTORS], fac_component[MFS_ND_MAX_FACTORS], fac_ycol[MFS_ND_MAX_FACTORS];
    const double* coef;      // [rows][D][D] or [B][rows][D][D]; blocks 0..4 = mu_0, mu_1, S_00, S_01, S_11
    const double* lik;       // [n_factors][MFS_MAX_LIK] or [B][n_factors][MFS_MAX_LIK]
    const double* ys;        // [B][T][ny]
    const uint64_t* seeds;   // [B]
    int n_mix, init_batched; // initial law: a mixture of n_mix Normals drawn on the device, or (n_mix = 0) given samples
    const double* mix_cumw;  // [n_mix]
    const double* mix_mean;  // [n_mix][2]
    const double* mix_chol;  // [n_mix][2][2], lower factors
    const double* init;      // [n][2] or [B][n][2]
    double* x;               // [B][2][n] the particles: propagated in place, read by the resampler
    double* x2;              // [B][2][n] the resampled particles (the host swaps x and x2 after every step)
    double* wscan;           // [B][n] block-local inclusive prefix sums of the weights
    double* wpart;           // [B][nblk] block totals of the weights
    double* woffs;           // [B][nblk] their exclusive prefix sums in index order
    double* wtot;            // [B] sum of the weights
    double* xpart;           // [B][2][nblk] block totals of the resampled particles, per component
    double* cpart;           // [B][3][nseg] segment totals of d_0 d_0, d_0 d_1, d_1 d_1, d = x' - mean
    double* out_samples;     // [B][T][n][2] or null
    double* out_means;       // [B][T][2]
    double* out_covs;        // [B][T][2][2]
};

// ---- Gaussian filters
struct GfArgs {
    int d, method;           // 1 or 2; MFS_GF_*
    int n_points, lanes;     // sigma points (0 for the EKF) and lanes per replicate (1 for the EKF)
    int T, B;
    // d = 1 (mfs_model_1d, MFS_TRANS_GAUSSIAN): coef [2][degree + 1] or [B][2][degree + 1]; lik [n_lik] or [B][n_lik]
    int umap, degree, coef_batched, lik_kind, n_lik, lik_batched;
    double mean_x_coef;
    // d = 2 (mfs_model_nd, MFS_ND_TRANS_GAUSSIAN): coef [rows][extent][extent], blocks 0..4 = mu_0, mu_1, S_00, S_01, S_11; one
    // likelihood factor of kind lik_kind on state component `component`, lik [MFS_MAX_LIK] or [B][MFS_MAX_LIK]
    int extent, component;
    const double* coef;
    const double* lik;
    const double* xi;        // [n_points][d]
    const double* w;         // [n_points]
    const double* m0;        // [d] or [B][d]
    const double* P0;        // [d][d] or [B][d][d]
    int init_batched;
    const double* ys;        // [B][T]
    double* out_means;       // [B][T][d] or null
    double* out_covs;        // [B][T][d][d] or null
    double* out_nells;       // [B][T], the running sum
    int32_t* out_first_nan;  // [B] or null
};

}  // namespace mfs
