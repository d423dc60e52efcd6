// likelihood.hpp -- the scalar measurement densities l(y | x) of the likelihood kinds of include/mfs_hip.h, each defined once.
// Two forms: `likelihood` with libm's exp / log (dense 1-D kernel, grid filter, particle filters), and `lik_density<SC>` with the
// in-line exponential / logarithm of device_util.hpp (the N-D kernels through likelihood_nd, likelihood_joint_nd and the joint
// factors of d = 3).  The fast 1-D kernels have the same arithmetic in a table form of their own (likelihood_fast, below).
#pragma once
#include "../../include/mfs_hip.h"
#include "device_util.hpp"

namespace mfs {

__device__ __forceinline__ double likelihood(const int kind, const double* __restrict__ lp, const double y,
                                             const double x) {
    if (kind == MFS_LIK_BERNOULLI_LOGISTIC) {
        const double z = lp[0] + x * (lp[1] + x * (lp[2] + x * lp[3]));
        const double p = 1.0 / (1.0 + exp(-z));
        return (y > 0.5) ? p : 1.0 - p;
    } else if (kind == MFS_LIK_POISSON_SOFTPLUS) {
        const double rate = log(1.0 + exp(lp[0] * x));
        return exp(poisson_log_pmf(y, rate, log(rate), log_factorial(y)));
    } else {
        const double r = y - (lp[0] * x + lp[1]);
        return exp(-0.5 * r * r / lp[2]) * rsqrt(6.283185307179586476925 * lp[2]);
    }
}

// the three kinds on a link value eta (var: the Gaussian's variance), with the in-line exponential / logarithm; SC = their
// scalar-constant form (fast_exp<true>: see there).  Bernoulli-logistic is mfs/multi_dims/ss_models.py:63-67
template <bool SC>
__device__ __forceinline__ double lik_density(const int kind, const double eta, const double var, const double y) {
    if (kind == MFS_LIK_BERNOULLI_LOGISTIC) {
        const double p = rcp_sat(1.0 + fast_exp<SC>(-eta));   // e^{-eta} may be +inf: p = 0, as 1 / (1 + inf) upstream
        return (y > 0.5) ? p : 1.0 - p;
    }
    if (kind == MFS_LIK_POISSON_SOFTPLUS) {
        const double rate = rate_floor(fast_log<SC>(1.0 + fast_exp<SC>(eta)));
        return fast_exp<SC>(poisson_log_pmf(y, rate, fast_log<SC>(rate), log_factorial(y)));
    }
    const double r = y - eta;
    return fast_exp<SC>(-0.5 * r * r * rcp_nr(var)) * rsq_nr(6.283185307179586476925 * var);
}

// a factor of ONE state component x in the N-D kernels: the kind's link value of x, then its density
__device__ __forceinline__ double likelihood_nd(const int kind, const double* __restrict__ lp, const double y,
                                                const double x) {
    if (kind == MFS_LIK_BERNOULLI_LOGISTIC) {
        return lik_density<true>(MFS_LIK_BERNOULLI_LOGISTIC, lp[0] + x * (lp[1] + x * (lp[2] + x * lp[3])), 0.0, y);
    }
    if (kind == MFS_LIK_POISSON_SOFTPLUS) return lik_density<true>(MFS_LIK_POISSON_SOFTPLUS, lp[0] * x, 0.0, y);
    return lik_density<true>(MFS_LIK_GAUSSIAN, fma(lp[0], x, lp[1]), lp[2], y);
}

// a factor of BOTH state components (fac_component = 2).  MFS_LIK_BEARING_GAUSSIAN: y ~ N(atan2(x_1, x_0), lp[0]) -- the
// bearing-only measurement of examples/2d_bearing_only.ipynb cell 7, norm.pdf(y, arctan2(x[1], x[0]), sd)
__device__ __forceinline__ double likelihood_joint_nd(const int kind, const double* __restrict__ lp, const double y,
                                                      const double x0, const double x1) {
    if (kind == MFS_LIK_BEARING_GAUSSIAN) return lik_density<true>(MFS_LIK_GAUSSIAN, atan2(x1, x0), lp[0], y);
    return __builtin_nan("");
}

// ---- the table form of the fast 1-D kernels
constexpr int kLfacMax = 32;   // log(y!) is tabulated in LDS for y = 0..kLfacMax

// likelihood parameters held by value: the fixed-traits one-wave builds read them from LDS once, before the time loop
struct LikRegs { double v[MFS_MAX_LIK]; };
__device__ __forceinline__ double lik_at(const double* lp, const int i) { return lp[i]; }
__device__ __forceinline__ double lik_at(const LikRegs* lp, const int i) { return lp->v[i]; }
__device__ __forceinline__ const double* lik_ptr(const double* lp) { return lp; }
__device__ __forceinline__ const double* lik_ptr(const LikRegs* lp) { return lp->v; }

// Poisson pmf with log(y!) looked up for the counts that actually occur (y <= 32) instead of a sum of logs per step
// (LP: double -- the parameters in the LDS staging area -- or LikRegs)
// (the density's arithmetic is lik_density's, kept as a separate function because merging the two changes the 1-D kernels' code)
template <class LP>
__device__ __forceinline__ double likelihood_fast(const int kind, const LP* __restrict__ lp,
                                                  const double* __restrict__ lfac, const double y, const double x) {
    if (kind == MFS_LIK_POISSON_SOFTPLUS) {
        const double rate = rate_floor(fast_log(1.0 + fast_exp(lik_at(lp, 0) * x)));
        const double lf = (y >= 0.0 && y <= (double)kLfacMax && y == floor(y)) ? lfac[(int)y] : log_factorial(y);
        return fast_exp(poisson_log_pmf(y, rate, fast_log(rate), lf));
    }
    if (kind == MFS_LIK_BERNOULLI_LOGISTIC) {
        const double z = lik_at(lp, 0) + x * (lik_at(lp, 1) + x * (lik_at(lp, 2) + x * lik_at(lp, 3)));
        const double p = rcp_sat(1.0 + fast_exp(-z));   // e^{-z} may be +inf: p = 0, as 1 / (1 + inf) upstream
        return (y > 0.5) ? p : 1.0 - p;
    }
    if (kind == MFS_LIK_GAUSSIAN) {
        const double r = y - fma(lik_at(lp, 0), x, lik_at(lp, 1));
        return fast_exp(-0.5 * r * r * rcp_nr(lik_at(lp, 2))) * rsq_nr(6.283185307179586476925 * lik_at(lp, 2));
    }
    return likelihood(kind, lik_ptr(lp), y, x);
}

// the parameters from registers (REGS) or from their LDS staging area
template <bool REGS>
__device__ __forceinline__ double likelihood_sel(const int kind, const LikRegs& lpr, const double* __restrict__ lp,
                                                 const double* __restrict__ lfac, const double y, const double x) {
    if constexpr (REGS) return likelihood_fast(kind, &lpr, lfac, y, x);
    else return likelihood_fast(kind, lp, lfac, y, x);
}

}  // namespace mfs
