// registry.hpp -- every launcher type and launcher table of the library, declared once.  The *_inst.hip translation units
// fill the tables from static registrars; capi.hip reads them.  A null launcher means "not compiled / does not exist".
// Host-only; the argument structs the launchers take are defined in kernel_args.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mfs_hip.h"
#include "kernel_args.hpp"

namespace mfs {

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

// ---- diagnostic: the shared device math and the likelihood forms (device_math_inst.hip), MFS_DM_* of include/mfs_hip.h
struct DeviceMathShape { int n_in, n_out; };
// rows of `in` and `out` a routine takes; {0, 0} for a code that names none
constexpr DeviceMathShape device_math_shape(const int fn) {
    return (fn < 0 || fn >= MFS_DM_COUNT) ? DeviceMathShape{0, 0}
         : (fn <= MFS_DM_LOG_FACTORIAL || fn == MFS_DM_LFAC_TABLE) ? DeviceMathShape{1, 1}
         : (fn == MFS_DM_HORNER) ? DeviceMathShape{2 + MFS_MAX_DEGREE + 1, 1}
         : (fn == MFS_DM_POLY2) ? DeviceMathShape{3 + MFS_ND_MAX_EXTENT_HI * MFS_ND_MAX_EXTENT_HI, 1}
         : (fn == MFS_DM_POLY2_GRAD) ? DeviceMathShape{3 + MFS_ND_MAX_EXTENT_HI * MFS_ND_MAX_EXTENT_HI, 3}
         : (fn == MFS_DM_CHOL2) ? DeviceMathShape{3, 4}
         : (fn == MFS_DM_LIK_DENSITY || fn == MFS_DM_LIK_DENSITY_SC) ? DeviceMathShape{4, 1}
         : (fn == MFS_DM_LIKELIHOOD_JOINT_ND) ? DeviceMathShape{MFS_MAX_LIK + 4, 1}
         : DeviceMathShape{MFS_MAX_LIK + 3, 1};
}
hipError_t launch_device_math(int fn, int n, const double* d_in, double* d_out, hipStream_t s);

// ---- N-D, d = 3: [N]
using FilterNd3Launch = hipError_t (*)(const FilterNd3Args&, int grid, hipStream_t);
using FilterNd3JointLaunch = hipError_t (*)(const FilterNd3Args&, const FilterNd3Joint&, int grid, hipStream_t);
struct Nd3Entry { FilterNd3Launch launch, launch_gauss; int S, Z, lds_bytes; FilterNd3JointLaunch joint, joint_gauss; };
extern Nd3Entry g_nd3_table[MFS_ND3_MAX_N + 1];   // defined in filternd3_inst.hip

// ---- brute-force grid filter (gridfilter_inst.hip): one build of each kernel, so plain launchers and no table.  Every
// matrix is row-major in a buffer padded to multiples of 64 (n_pad, ldp); the GEMM takes padded sizes only and refuses
// anything else, and C must not alias A or B.
constexpr int kGridTile = 64;   // the GEMM's block tile in M and N; every padded dimension is a multiple of it
constexpr int kGridBK = 16;     // ... and its k-slice

inline int grid_pad(const int v) { return (v + kGridTile - 1) / kGridTile * kGridTile; }

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

hipError_t launch_pf_init(const PfArgs& a, hipStream_t s);
hipError_t launch_pf_propagate(const PfArgs& a, hipStream_t s);
hipError_t launch_pf_offsets(const PfOffsetsArgs& a, hipStream_t s);
hipError_t launch_pf_resample(const PfArgs& a, hipStream_t s);
hipError_t launch_pf_cf(const PfArgs& a, hipStream_t s);
hipError_t launch_pf_finalize(const PfArgs& a, hipStream_t s);
hipError_t launch_pf_draws(uint64_t seed, int t, int tag, int draw, int count, double* d_uniform, double* d_normal, hipStream_t s);

// ---- bootstrap particle filter, d = 2 (particle_nd_inst.hip).  The same five launches per measurement, the same constants
// and the same `offsets` kernel (launch_pf_offsets with a PfOffsetsArgs).
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

int gf_lds_bytes(const GfArgs& a);   // dynamic LDS of one block
hipError_t launch_gauss_filter(const GfArgs& a, hipStream_t s);

}  // namespace mfs
