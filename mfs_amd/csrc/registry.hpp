// registry.hpp -- every launcher type and launcher table of the library, declared once.  The *_inst.hip translation units
// fill the tables from static registrars; capi.hip reads them.  A null launcher means "not compiled / does not exist".
// Host-only: the argument structs are only named here (their definitions live with the kernels; the grid filter's, the
// particle filter's and the Gaussian filters' are the exceptions).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mfs_hip.h"

namespace mfs {

struct Filter1dArgs;
struct Quad1dArgs;
struct Cf1dArgs;
struct Filter1dGradArgs;
struct FilterNdArgs;
struct FilterNd3Args;
struct FilterNd3Joint;

// ---- 1-D: dense (LDS-tile) and fast (register-resident) paths
using Filter1dLaunch = hipError_t (*)(const Filter1dArgs&, int grid, int lds_bytes, hipStream_t);
using Quad1dLaunch = hipError_t (*)(const Quad1dArgs&, int grid, int lds_bytes, hipStream_t);
using Filter1dFastLaunch = hipError_t (*)(const Filter1dArgs&, int grid, int lds_doubles_per_filter, hipStream_t);
using Cf1dLaunch = hipError_t (*)(const Cf1dArgs&, int grid, int lds, hipStream_t);

struct KernelEntry {
    Filter1dLaunch filter;       // dense slots only
    Quad1dLaunch quad;
    int lds_doubles_per_filter;  // dense: complete; fast: fixed part, the model table is added at launch
    int waves_per_block;
    int lanes_per_filter;
};

// slots per N: [0..2] dense path with G = 16 / 32 / 64, [3 + gi] fast path of lane group gi
constexpr int kSlots = 7;
extern KernelEntry g_table[MFS_MAX_N + 1][kSlots];   // defined in capi.hip, filled by filter1d_inst.hip

// lane groups of the fast path: gi 0..2 = 16 / 32 / 64 lanes per filter, gi 3 = 8 lanes (eight filters per wavefront)
constexpr int group_lanes(const int gi) { return (gi == 3) ? 8 : 16 << gi; }
// the default group of an order: the smallest that holds the N + 1 rows of the extended Hankel matrix
constexpr int default_group(const int N) { return (N + 1 <= 8) ? 3 : (N + 1 <= 16) ? 0 : (N + 1 <= 32) ? 1 : 2; }

// specialised one-wave builds of the fast kernel (filter1d_fast.hpp, SPEC): kSpecShapes table shapes
constexpr int kSpecShapes = 4;
// slot of a table shape among them (-1 = normal closure, 2 / 4 / 6 = operator terms), or -1 if the shape has no such build
constexpr int spec_shape_index(const int spec) { return (spec == -1) ? 0 : (spec == 2) ? 1 : (spec == 4) ? 2 : (spec == 6) ? 3 : -1; }

// fixed step traits of the specialised builds (filter1d_fast.hpp, StepTraits): the (mode, u-map, likelihood) combinations a
// shipped model reaches with a one-wave build.  The value is what mfs_plan_1d_kernel_traits reports (MFS_TRAITS_*); 0 = the
// three stay run-time values.
constexpr int kTraitSets = 2;
constexpr int traits_index(const int mode, const int umap, const int lik_kind) {
    return (mode != MFS_MODE_CENTRAL) ? MFS_TRAITS_RUNTIME
         : (umap == MFS_U_TANH && lik_kind == MFS_LIK_BERNOULLI_LOGISTIC) ? MFS_TRAITS_CENTRAL_TANH_BERNOULLI
         : (umap == MFS_U_IDENTITY && lik_kind == MFS_LIK_GAUSSIAN) ? MFS_TRAITS_CENTRAL_IDENTITY_GAUSSIAN
         : MFS_TRAITS_RUNTIME;
}

// placement counters of the partner-wave variant: {workgroups checked, workgroups whose waves w and w + 4 did not share a SIMD},
// over the launches of the process.  Each translation unit with partner kernels holds its own copy and registers a reader.
using PartnerPlacementRead = hipError_t (*)(unsigned long long counts[2]);

// what the fast path has for one (N, lane group) beside its g_table slot
struct FastEntry {
    Filter1dFastLaunch filter;             // the plain build
    Filter1dFastLaunch wide;               // one-wave-per-SIMD register budget (the orders that spill at two; default group only)
    Filter1dFastLaunch ext, ext_wide;      // extended variant (stable = 1, odd moment counts; default group only)
    Filter1dFastLaunch spec[kSpecShapes];  // [spec_shape_index]: specialised one-wave builds (default group of N = 14..16)
    Filter1dFastLaunch spec_traits[kSpecShapes][kTraitSets];   // [spec_shape_index][traits_index - 1]: the same with fixed step
                                                               // traits; null where the pair has no build
    Filter1dFastLaunch partner[kSpecShapes][kTraitSets];       // the partner-wave variant of spec_traits (filter1d_partner.hpp:
    int partner_doubles;                                       // N = 14, 15), and its extra LDS doubles per filter
    PartnerPlacementRead partner_placement;                    // reader of the placement counters of the unit that holds them
    Quad1dLaunch quad_ext;                 // quadrature entry with stable = 1
    Cf1dLaunch cf;                         // characteristic function
    int ext_shift;                         // extra LDS doubles per filter of the extended variant
    int quad_ext_lds;                      // LDS doubles per filter of quad_ext
};
extern FastEntry g_fast[MFS_MAX_N + 1][4];   // defined in capi.hip, filled by filter1d_inst.hip (spec: filter1d_spec_inst.hip,
                                             // partner: filter1d_partner_inst.hip)

// geometry of the partner-wave variant: 512-thread workgroups, four main waves of four filters and their four partner waves;
// dynamic LDS = the main waves' tiles (the one-wave builds') + the partner's tile per filter, within the CU's 160 KiB
constexpr int kPartnerFilters = 16;
constexpr int kPartnerLdsMax = 160 * 1024;
constexpr int partner_lds_bytes(const int lds_doubles_per_filter, const int partner_doubles) {
    return kPartnerFilters * (lds_doubles_per_filter + partner_doubles) * 8;
}

// ---- 1-D gradient: [N][n_par]
using Filter1dGradLaunch = hipError_t (*)(const Filter1dGradArgs&, int n_filters, hipStream_t);
constexpr int kGradMaxN = 16, kGradMaxP = 4;
extern Filter1dGradLaunch g_grad_table[kGradMaxN + 1][kGradMaxP + 1];   // defined in filter1d_grad_inst.hip

// ---- N-D, d = 2: [N]
using FilterNdLaunch = hipError_t (*)(const FilterNdArgs&, int grid, hipStream_t);
struct NdEntry { FilterNdLaunch launch, launch_gauss, launch_hi, launch_joint; int S, Z, lds_bytes, carry_doubles; };
constexpr int kNdMaxN = 7;
extern NdEntry g_nd_table[kNdMaxN + 1];   // defined in filternd_inst.hip
hipError_t launch_elementary(int which, int n, const double* d_x, double* d_out, hipStream_t s);   // filternd_inst.hip

// ---- N-D, d = 3: [N]
using FilterNd3Launch = hipError_t (*)(const FilterNd3Args&, int grid, hipStream_t);
using FilterNd3JointLaunch = hipError_t (*)(const FilterNd3Args&, const FilterNd3Joint&, int grid, hipStream_t);
struct Nd3Entry { FilterNd3Launch launch, launch_gauss; int S, Z, lds_bytes; FilterNd3JointLaunch joint, joint_gauss; };
extern Nd3Entry g_nd3_table[MFS_ND3_MAX_N + 1];   // defined in filternd3_inst.hip

// ---- brute-force grid filter (gridfilter_inst.hip): one build of each kernel, so plain launchers and no table.  Every
// matrix is row-major in a buffer padded to multiples of 64 (n_pad, ldp); the GEMM takes padded sizes only and refuses
// anything else, and C must not alias A or B.  (GridUpdateArgs is defined here, not just named: its kernels are not templates,
// so their header can be included by gridfilter_inst.hip alone.)
constexpr int kGridTile = 64;   // the GEMM's block tile in M and N; every padded dimension is a multiple of it
constexpr int kGridBK = 16;     // ... and its k-slice

inline int grid_pad(const int v) { return (v + kGridTile - 1) / kGridTile * kGridTile; }

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
hipError_t launch_grid_build_k(int n, int n_pad, const double* d_xs, const double* d_mean, const double* d_sd,
                               const double* d_w, double* d_K, hipStream_t s);
hipError_t launch_grid_init_p(int n, int n_pad, int B, int ldp, const double* d_init, int init_batched, double* d_P,
                              hipStream_t s);
hipError_t launch_grid_gemm(int M, int N, int Kd, const double* d_A, const double* d_B, double* d_C, hipStream_t s);
hipError_t launch_grid_update(const GridUpdateArgs& a, hipStream_t s);
// the characteristic function of densities on the grid: the table of weighted cosines and sines ([2 m_pad][n_pad], or its
// transpose [n_pad][2 m_pad]), and the two stores of a product with it -- the filter's ([2 m_pad][ldp] -> place `slot` of a
// block of [B][S][nz] pairs, NaN where first_nan[b] >= 0) and the one of densities by rows ([rows][2 m_pad] -> [rows][nz] pairs)
hipError_t launch_grid_cf_table(int n, int nz, int n_pad, int m_pad, int transposed, const double* d_xs, const double* d_w,
                                const double* d_zs, double* d_E, hipStream_t s);
hipError_t launch_grid_cf_store(int nz, int B, int m_pad, int ldp, int S, int slot, const double* d_C, const int32_t* d_first_nan,
                                double* d_out, hipStream_t s);
hipError_t launch_grid_cf_store_rows(int rows, int nz, int m_pad, const double* d_C, double* d_out, hipStream_t s);

// ---- bootstrap particle filter (particle_inst.hip): plain launchers, like the grid filter's.  One measurement is five launches
// on one stream -- propagate (with the block scan of the weights), offsets, resample, cf (with the variance), finalize -- and
// every sum's order is fixed by n and these constants alone.
constexpr int kPfThreads = 256;                    // threads per block of every particle kernel
constexpr int kPfItems = 4;                        // particles per thread
constexpr int kPfChunk = kPfThreads * kPfItems;    // particles per block: the unit of the weight scan and of the x' partial sums
constexpr int kPfSeg = 4 * kPfChunk;               // particles per block of the cf / variance pass
constexpr int kPfMaxF = 8;                         // frequencies per thread of the cf pass (its rotation recurrence restarts there)

inline int pf_blocks(const int n) { return (n + kPfChunk - 1) / kPfChunk; }
inline int pf_segments(const int n) { return (n + kPfSeg - 1) / kPfSeg; }

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
hipError_t launch_pf_init(const PfArgs& a, hipStream_t s);
hipError_t launch_pf_propagate(const PfArgs& a, hipStream_t s);
hipError_t launch_pf_offsets(const PfOffsetsArgs& a, hipStream_t s);
hipError_t launch_pf_resample(const PfArgs& a, hipStream_t s);
hipError_t launch_pf_cf(const PfArgs& a, hipStream_t s);
hipError_t launch_pf_finalize(const PfArgs& a, hipStream_t s);
hipError_t launch_pf_draws(uint64_t seed, int t, int tag, int draw, int count, double* d_uniform, double* d_normal, hipStream_t s);

// ---- bootstrap particle filter, d = 2 (particle_nd_inst.hip).  The same five launches per measurement, the same constants
// and the same `offsets` kernel (launch_pf_offsets with a PfOffsetsArgs); the particles are [B][2][n], component-major, so
// every particle pass is coalesced.
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
hipError_t launch_pfnd_init(const PfNdArgs& a, hipStream_t s);
hipError_t launch_pfnd_propagate(const PfNdArgs& a, hipStream_t s);
hipError_t launch_pfnd_resample(const PfNdArgs& a, hipStream_t s);
hipError_t launch_pfnd_cov(const PfNdArgs& a, hipStream_t s);
hipError_t launch_pfnd_finalize(const PfNdArgs& a, hipStream_t s);

// ---- Gaussian filters (gaussfilter_inst.hip): the Gauss--Hermite / cubature sigma-point filter and the extended Kalman filter,
// d = 1 and d = 2, the whole time loop in one launch.  A group of gf_lanes(n_points) lanes owns a replicate (one lane for the
// EKF); a block is one wavefront, so it holds kGfThreads / lanes replicates.
constexpr int kGfThreads = 64;

// lanes per replicate of the sigma-point filter: the smallest power of two >= n_points, at most a wavefront.  It depends on
// n_points alone, never on B, so a replicate's sums run in the same order whatever the batch.
inline int gf_lanes(const int n_points) {
    int L = 1;
    while (L < n_points && L < kGfThreads) L <<= 1;
    return L;
}

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
int gf_lds_bytes(const GfArgs& a);   // dynamic LDS of one block
hipError_t launch_gauss_filter(const GfArgs& a, hipStream_t s);

}  // namespace mfs
