// device_math_inst.hip -- diagnostic: every routine of the shared device layer (device_util.hpp, likelihood.hpp) on arrays, one
// thread per element and one kernel per routine (MFS_DM_* of include/mfs_hip.h), so that the tests can compare each of them with
// exact arithmetic apart from any filter.  No kernel family's header is included.
#include <utility>

#include "device_util.hpp"
#include "likelihood.hpp"
#include "registry.hpp"

namespace mfs {

constexpr int kDmThreads = 256;

// in [n_in][n], out [n_out][n]; integer arguments travel as doubles
template <int FN>
__global__ void __launch_bounds__(kDmThreads) device_math_kernel(const int n, const double* __restrict__ in, double* __restrict__ out) {
    constexpr bool kTable = (FN == MFS_DM_LIKELIHOOD_FAST || FN == MFS_DM_LIKELIHOOD_FAST_REGS || FN == MFS_DM_LFAC_TABLE);
    __shared__ double lfac[kLfacMax + 1];
    if constexpr (kTable) {   // the log(y!) table as the fast 1-D kernels stage it
        for (int e = threadIdx.x; e <= kLfacMax; e += kDmThreads) lfac[e] = log_factorial((double)e);
        __syncthreads();
    }
    const int i = blockIdx.x * kDmThreads + threadIdx.x;
    if (i >= n) return;
    auto arg = [&](const int j) { return in[(size_t)j * n + i]; };
    auto put = [&](const int j, const double v) { out[(size_t)j * n + i] = v; };

    if constexpr (FN == MFS_DM_EXP) put(0, fast_exp<false>(arg(0)));
    else if constexpr (FN == MFS_DM_EXP_SC) put(0, fast_exp<true>(arg(0)));
    else if constexpr (FN == MFS_DM_TANH) put(0, fast_tanh(arg(0)));
    else if constexpr (FN == MFS_DM_LOG) put(0, fast_log<false>(arg(0)));
    else if constexpr (FN == MFS_DM_LOG_SC) put(0, fast_log<true>(arg(0)));
    else if constexpr (FN == MFS_DM_RCP_NR) put(0, rcp_nr(arg(0)));
    else if constexpr (FN == MFS_DM_RCP_SAT) put(0, rcp_sat(arg(0)));
    else if constexpr (FN == MFS_DM_RSQ_NR) put(0, rsq_nr(arg(0)));
    else if constexpr (FN == MFS_DM_LOG_FACTORIAL) put(0, log_factorial(arg(0)));
    else if constexpr (FN == MFS_DM_LFAC_TABLE) {
        const int e = (int)arg(0);
        put(0, (e >= 0 && e <= kLfacMax) ? lfac[e] : __builtin_nan(""));
    } else if constexpr (FN == MFS_DM_HORNER) {
        double row[MFS_MAX_DEGREE + 1];
        for (int j = 0; j <= MFS_MAX_DEGREE; ++j) row[j] = arg(2 + j);
        const int degree = min(max((int)arg(0), 0), MFS_MAX_DEGREE);
        put(0, horner(row, degree, arg(1)));
    } else if constexpr (FN == MFS_DM_POLY2 || FN == MFS_DM_POLY2_GRAD) {
        constexpr int HI = MFS_ND_MAX_EXTENT_HI;
        double c[HI * HI];
        for (int j = 0; j < HI * HI; ++j) c[j] = arg(3 + j);
        const int D = min(max((int)arg(0), 1), HI);
        if constexpr (FN == MFS_DM_POLY2) {
            put(0, gf_poly2(c, D, arg(1), arg(2)));
        } else {
            double d0, d1;
            put(0, gf_poly2_grad(c, D, arg(1), arg(2), d0, d1));
            put(1, d0);
            put(2, d1);
        }
    } else if constexpr (FN == MFS_DM_CHOL2) {
        double l00, l10, l11;
        const bool ok = gf_chol2(arg(0), arg(1), arg(2), l00, l10, l11);
        put(0, l00);
        put(1, l10);
        put(2, l11);
        put(3, ok ? 1.0 : 0.0);
    } else if constexpr (FN == MFS_DM_LIK_DENSITY) put(0, lik_density<false>((int)arg(0), arg(1), arg(2), arg(3)));
    else if constexpr (FN == MFS_DM_LIK_DENSITY_SC) put(0, lik_density<true>((int)arg(0), arg(1), arg(2), arg(3)));
    else {
        const int kind = (int)arg(0);
        double lp[MFS_MAX_LIK];
        for (int j = 0; j < MFS_MAX_LIK; ++j) lp[j] = arg(1 + j);
        const double y = arg(1 + MFS_MAX_LIK), x = arg(2 + MFS_MAX_LIK);
        if constexpr (FN == MFS_DM_LIKELIHOOD) put(0, likelihood(kind, lp, y, x));
        else if constexpr (FN == MFS_DM_LIKELIHOOD_ND) put(0, likelihood_nd(kind, lp, y, x));
        else if constexpr (FN == MFS_DM_LIKELIHOOD_JOINT_ND) put(0, likelihood_joint_nd(kind, lp, y, x, arg(3 + MFS_MAX_LIK)));
        else if constexpr (FN == MFS_DM_LIKELIHOOD_FAST) put(0, likelihood_fast(kind, (const double*)lp, lfac, y, x));
        else {
            static_assert(FN == MFS_DM_LIKELIHOOD_FAST_REGS, "a routine without a kernel");
            LikRegs regs;
            for (int j = 0; j < MFS_MAX_LIK; ++j) regs.v[j] = lp[j];
            put(0, likelihood_fast(kind, (const LikRegs*)&regs, lfac, y, x));
        }
    }
}

template <int FN>
static hipError_t dm_launch(const int n, const double* d_in, double* d_out, hipStream_t s) {
    hipLaunchKernelGGL((device_math_kernel<FN>), dim3((n + kDmThreads - 1) / kDmThreads), dim3(kDmThreads), 0, s, n, d_in, d_out);
    return hipGetLastError();
}

template <int... FN>
static hipError_t dm_dispatch(std::integer_sequence<int, FN...>, const int fn, const int n, const double* d_in, double* d_out,
                              hipStream_t s) {
    hipError_t e = hipErrorInvalidValue;
    (void)((fn == FN ? (e = dm_launch<FN>(n, d_in, d_out, s), true) : false) || ...);
    return e;
}

hipError_t launch_device_math(int fn, int n, const double* d_in, double* d_out, hipStream_t s) {
    return dm_dispatch(std::make_integer_sequence<int, MFS_DM_COUNT>{}, fn, n, d_in, d_out, s);
}

}  // namespace mfs
