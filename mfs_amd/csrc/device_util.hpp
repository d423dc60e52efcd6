// device_util.hpp -- device helpers that belong to no kernel family: compile-time loops, group reductions by shuffle, single
// DPP / min / max instructions, Newton-refined reciprocals, the in-line exp / tanh / log, log(y!), and the small polynomial and
// 2 x 2 Cholesky evaluators several families share.  Every kernel header includes this one instead of another family's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace mfs {

template <int I, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < E) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, E>(f);
    }
}

__device__ __forceinline__ bool finite(double v) { return fabs(v) <= 1.79769313486231570e308; }

__device__ __forceinline__ void wave_sync() {
    // Orders this wave's LDS traffic for cross-lane hand-offs inside one wavefront: LDS executes a wave's
    // instructions in order, so all that is needed is to stop the compiler from moving accesses across this point.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int G>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
    return v;
}

template <int G>
__device__ __forceinline__ int group_or(int v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v |= __shfl_xor(v, o, G);
    return v;
}

// v_min_f64 / v_max_f64 as single instructions: fmin() / fmax() compile to a canonicalising v_max_f64 x, x in front of
// each (signalling-NaN quieting), which doubles the cost of the Gershgorin bounds; the operands here are results of
// arithmetic, and a NaN among them has already poisoned the rule.
__device__ __forceinline__ double vmin_f64(const double a, const double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double vmax_f64(const double a, const double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// v of the lane that the DPP control CTRL names (quad permutations, row mirrors): two v_mov_b32_dpp
template <int CTRL>
__device__ __forceinline__ double dpp_move(double v) {
    // (bound_ctrl set: these patterns give every lane a source, and with it the compiler needs no pass-through value)
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double rcp_nr(const double v) {
    double y = __builtin_amdgcn_rcp(v);
    y = fma(fma(-v, y, 1.0), y, y);
    y = fma(fma(-v, y, 1.0), y, y);
    return y;
}

// the same, but 1 / (+-inf) = 0 like a true divide (the Newton steps alone turn it into NaN)
__device__ __forceinline__ double rcp_sat(const double v) {
    const double y0 = __builtin_amdgcn_rcp(v);
    double y = fma(fma(-v, y0, 1.0), y0, y0);
    y = fma(fma(-v, y, 1.0), y, y);
    return (y0 == 0.0) ? y0 : y;
}

__device__ __forceinline__ double rsq_nr(const double v) {
    // (-0.5 y v, in this order: halving y is exact, halving a v below 2^-1021 drops its last bit -- down to all of them at
    //  2^-1074, where the result came out 2.25 times too large; for every larger v the product rounds to the same bits either way)
    double y = __builtin_amdgcn_rsq(v);
    y = fma(y, fma(-0.5 * y * v, y, 0.5), y);
    y = fma(y, fma(-0.5 * y * v, y, 0.5), y);
    return y;
}

// ---- elementary functions of the step, written for instruction count (the kernel is VALU-issue bound on one wave per
// SIMD): ~22 / 33 / 34 VALU instructions for exp / tanh / log against 34 / 155 / 90 for the ocml routines.  Absolute
// accuracy ~1-2 ulp of the result's magnitude scale; tanh keeps ABSOLUTE (not relative) accuracy near zero, which is
// what a polynomial in tanh x needs.
// (SC: the polynomial's constants as SCALAR operands of `v_fma_f64`.  The plain form compiles to `v_fmac_f64`, whose
//  addend is the destination, so every constant is first copied into a vector register pair -- loop-invariant copies that
//  get hoisted out of the time loop.  The 1-D kernels have the registers for that; the N-D kernel does not, spilled them and
//  reloaded each one from scratch between two dependent multiply-adds: ten serialised `s_waitcnt vmcnt(0)` per exponential.)
template <bool SC>
__device__ __forceinline__ double fma_const(const double p, const double r, const double c) {
    if constexpr (SC) {
        double o;
        asm("v_fma_f64 %0, %1, %2, %3" : "=v"(o) : "v"(p), "v"(r), "s"(c));
        return o;
    } else {
        return fma(p, r, c);
    }
}
// (Default of the 1-D kernels: off.  MFS_EXP_SC=1 frees ~20 vector registers there -- N = 7: 229 -> 207 -- but they have no
//  spills to cure and the pass times do not move: headline 6.76 against 6.69 ms, config-4 shard 54.3 against 54.6.)
#ifndef MFS_EXP_SC
#define MFS_EXP_SC 0
#endif
template <bool SC = (MFS_EXP_SC != 0)>
__device__ __forceinline__ double fast_exp(const double y) {
    // e^y = 2^k e^r, k = rint(y / ln 2), |r| <= ln 2 / 2, Taylor to degree 13 (r^14 / 14! < 5e-18)
    const double yc = vmin_f64(vmax_f64(y, -745.5), 710.0);     // e^710 = +inf as in libm (the clamp would swallow a NaN: restored below)
    const double k = __builtin_rint(yc * 1.4426950408889634);
    double r = fma(k, -0.6931471803691238, yc);                  // ln 2 split: hi part has 21 trailing zero bits
    r = fma(k, -1.9082149292705877e-10, r);
    double p = 1.6059043836821613e-10;                           // 1 / 13!
    p = fma_const<SC>(p, r, 2.08767569878681e-09);
    p = fma_const<SC>(p, r, 2.505210838544172e-08);
    p = fma_const<SC>(p, r, 2.755731922398589e-07);
    p = fma_const<SC>(p, r, 2.7557319223985893e-06);
    p = fma_const<SC>(p, r, 2.48015873015873e-05);
    p = fma_const<SC>(p, r, 0.0001984126984126984);
    p = fma_const<SC>(p, r, 0.001388888888888889);
    p = fma_const<SC>(p, r, 0.008333333333333333);
    p = fma_const<SC>(p, r, 0.041666666666666664);
    p = fma_const<SC>(p, r, 0.16666666666666666);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    const double e = ldexp(p, (int)k);
    return (y != y) ? y : e;
}

__device__ __forceinline__ double fast_tanh(const double x) {
    const double a2 = vmin_f64(fabs(x) + fabs(x), 40.0);        // tanh(20) rounds to 1
    const double e = fast_exp(a2);
    const double t = fma(-2.0, rcp_nr(e + 1.0), 1.0);            // 1 - 2 / (e^{2|x|} + 1)
    return (x != x) ? x : copysign(t, x);
}

// natural logarithm of a positive finite number (anything else gives a non-finite result, which is all the caller needs:
// a non-finite negative log-likelihood poisons the replicate)
template <bool SC = (MFS_EXP_SC != 0)>
__device__ __forceinline__ double fast_log(const double v) {
    // v = m 2^e, m in [0.5, 1): ln m from the fp32 hardware log as a seed y0 and one exact correction
    // ln m = y0 + log1p(m e^{-y0} - 1), |m e^{-y0} - 1| ~ 1e-7
    const double m = __builtin_amdgcn_frexp_mant(v);
    const int ex = __builtin_amdgcn_frexp_exp(v);
    const double y0 = (double)(__builtin_amdgcn_logf((float)m) * 0.6931471805599453f);
    const double d = fma(m, fast_exp<SC>(-y0), -1.0);
    const double lnm = y0 + fma(-0.5 * d, d, d);
    const double r = fma((double)ex, 0.6931471805599453, lnm);
    const double inf = __builtin_inf();
    return (v == 0.0) ? -inf : (v == inf) ? inf : r;      // log 0 = -inf, log inf = inf as in libm
}

// log(y!) for a Poisson count y (a non-negative integer stored as a double).  ocml's lgamma costs ~130 VGPRs when
// inlined into the hot loop; counts are small, so a short sum of logs (exact to rounding) does the job, with the
// Stirling series taking over for large y where it is accurate to < 1 ulp.
__device__ __forceinline__ double log_factorial(const double y) {
    if (y < 32.5) {
        double acc = 0.0;
        for (double k = 2.0; k <= y + 0.5; k += 1.0) acc += log(k);
        return acc;
    }
    const double z = y + 1.0, iz = 1.0 / z, iz2 = iz * iz;
    const double series = iz * (1.0 / 12.0 - iz2 * (1.0 / 360.0 - iz2 * (1.0 / 1260.0 - iz2 * (1.0 / 1680.0 - iz2 * (1.0 / 1188.0)))));
    return (z - 0.5) * log(z) - z + 0.91893853320467274178 + series;
}

// The exponent of the Poisson pmf, y log(rate) - rate - log(y!), from log(rate) as the caller's logarithm gave it.  At y = 0
// the first term is dropped, as xlogy does upstream: the softplus rate underflows to 0 (link below -36.8) or overflows to
// +inf (link above 710), and 0 * log(rate) would be NaN where the pmf is 1 and 0.  (The factor is replaced, not the product:
// the multiply-add the expression contracts to stays the one it was, and with it every finite result.)
__device__ __forceinline__ double poisson_log_pmf(const double y, const double rate, const double log_rate, const double lfac) {
    const double lr = (y == 0.0) ? 0.0 : log_rate;
    return y * lr - rate - lfac;
}

// The softplus rate of the in-line logarithm, kept non-negative: fast_log(1.0) is -2^-53, not 0 (its two halves cancel to the
// last bit but one), and the logarithm of that rate is NaN for every count.  A NaN rate stays NaN.
__device__ __forceinline__ double rate_floor(const double rate) { return (rate < 0.0) ? 0.0 : rate; }

// ---- polynomials and the 2 x 2 Cholesky factor
__device__ __forceinline__ double horner(const double* __restrict__ row, const int degree, const double u) {
    double acc = row[degree];
    for (int j = degree - 1; j >= 0; --j) acc = fma(acc, u, row[j]);
    return acc;
}

// sum_{a, b < D} c[a][b] x0^a x1^b by nested Horner
__device__ __forceinline__ double gf_poly2(const double* __restrict__ c, const int D, const double x0, const double x1) {
    double acc = 0.0;
    for (int a = D - 1; a >= 0; --a) {
        double row = c[a * D + D - 1];
        for (int b = D - 2; b >= 0; --b) row = row * x1 + c[a * D + b];
        acc = acc * x0 + row;
    }
    return acc;
}

// the same with both partial derivatives
__device__ __forceinline__ double gf_poly2_grad(const double* __restrict__ c, const int D, const double x0, const double x1,
                                                double& d0, double& d1) {
    double acc = 0.0;
    d0 = 0.0;
    d1 = 0.0;
    for (int a = D - 1; a >= 0; --a) {
        double row = c[a * D + D - 1], drow = 0.0;
        for (int b = D - 2; b >= 0; --b) {
            drow = drow * x1 + row;
            row = row * x1 + c[a * D + b];
        }
        d0 = d0 * x0 + acc;
        acc = acc * x0 + row;
        d1 = d1 * x0 + drow;
    }
    return acc;
}

// a legal Cholesky pivot: zero is (a point mass, as in the reference), negative and non-finite are not
__device__ __forceinline__ bool gf_pivot_ok(const double v) { return v >= 0.0 && finite(v); }

// lower Cholesky factor of [[p00, p01], [p01, p11]] in closed form; false if a pivot is negative or not finite.  A zero
// second pivot is legal (P = diag(v, 0)); a zero first pivot is not: l10 = p01 / 0 is NaN or +-inf, and so is the second pivot
__device__ __forceinline__ bool gf_chol2(const double p00, const double p01, const double p11, double& l00, double& l10,
                                         double& l11) {
    l00 = sqrt(p00);
    l10 = p01 / l00;
    const double d1 = p11 - l10 * l10;
    l11 = sqrt(d1);
    return gf_pivot_ok(p00) && gf_pivot_ok(d1);
}

}  // namespace mfs
