// gaussfilter_kernel.hpp -- hand-written HIP for gfx950 (MI355X): the Gaussian filters of mfs/classical_filters_smoothers/gfs.py,
// the sigma-point filter (sgp_filter :503-551 = _sgp_prediction :100-135 + _sgp_update :138-183, with any SigmaPoints rule) and
// the extended Kalman filter (ekf :317-362), for B replicates of a d = 1 or d = 2 state and a scalar measurement, in fp64.
// include/mfs_hip.h (mfs_gaussian_filter_1d / _nd) states the step; the whole time loop runs inside one launch.
//
// Mapping.  A block is one wavefront.  A group of L lanes owns a replicate, L = gf_lanes(n_points) (registry.hpp): lane l takes
// the sigma points l, l + L, l + 2 L, ... in that order, the group's partial sums meet in a butterfly (__shfl_xor inside the
// group), after which every lane holds the same bits, and the scalar tail of the step -- Cholesky factor, gain, update -- is
// computed redundantly by all of them.  Lane 0 stores.  The order of every sum is fixed by n_points alone and there are no
// atomics, so a replicate returns the same bits alone and in any batch.  The EKF has nothing to sum: one lane per replicate.
// Points, weights and shared model tables are staged in LDS once per block; per-replicate tables (coef_batched / lik_batched)
// once per group.  A group past the batch recomputes replicate B - 1 and stores nothing, so every lane reaches every shuffle.
//
// NaN rule (the reference's Cholesky of a non-positive-definite matrix is NaN): a pivot that is negative or not finite, or an
// innovation variance S that is not finite and > 0, or a measurement y_t that is not finite, makes mean, covariance and nell
// NaN; NaN then fails the same tests at every later step, so the replicate stays NaN, and the first such step is its first_nan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfs_hip.h"
#include "device_util.hpp"   // finite, group_sum, gf_pivot_ok, gf_poly2, gf_poly2_grad, gf_chol2
#include "registry.hpp"      // GfArgs (kernel_args.hpp), kGfThreads

namespace mfs {

// ---------------------------------------------------------------------------------------------------------------
// measurement moments: mean h(x), variance Xi(x) and (DERIV) d h / d x of the likelihood kinds of include/mfs_hip.h
// ---------------------------------------------------------------------------------------------------------------
struct GfLik { double l0, l1, l2, l3; };
struct GfMeas { double h, xi, dh; };

template <bool DERIV>
__device__ __forceinline__ GfMeas gf_measure(const int kind, const GfLik& p, const double x) {
    GfMeas r;
    if (kind == MFS_LIK_BERNOULLI_LOGISTIC) {
        // q(x) of a few thousand either way: exp overflows to inf, 1 / (1 + inf) = 0, and p (1 - p) = 0; no NaN
        const double z = p.l0 + x * (p.l1 + x * (p.l2 + x * p.l3));
        const double pr = 1.0 / (1.0 + exp(-z));
        r.h = pr;
        r.xi = pr * (1.0 - pr);
        r.dh = DERIV ? r.xi * (p.l1 + x * (2.0 * p.l2 + x * (3.0 * p.l3))) : 0.0;
    } else if (kind == MFS_LIK_POISSON_SOFTPLUS) {
        const double z = p.l0 * x;
        const double rate = fmax(z, 0.0) + log1p(exp(-fabs(z)));
        r.h = rate;
        r.xi = rate;
        r.dh = DERIV ? p.l0 / (1.0 + exp(-z)) : 0.0;
    } else {
        r.h = p.l0 * x + p.l1;
        r.xi = p.l2;
        r.dh = p.l0;
    }
    return r;
}

__device__ __forceinline__ GfLik gf_load_lik(const double* __restrict__ lk, const int n_lik) {
    GfLik p;
    p.l0 = lk[0];
    p.l1 = (n_lik > 1) ? lk[1] : 0.0;
    p.l2 = (n_lik > 2) ? lk[2] : 0.0;
    p.l3 = (n_lik > 3) ? lk[3] : 0.0;
    return p;
}

// ---------------------------------------------------------------------------------------------------------------
// d = 1
// ---------------------------------------------------------------------------------------------------------------
// mu(x) = c x + P_m(u), var(x) = P_v(u), u = x or tanh x; coef = [2][degree + 1] in ascending powers.  DERIV: also d mu / d x =
// c + P_m'(u) u', u' = 1 - u^2 for the tanh map
template <bool DERIV>
__device__ __forceinline__ void gf_trans_1d(const double* __restrict__ coef, const int degree, const int umap, const double c,
                                            const double x, double& mu, double& var, double& dmu) {
    const double u = (umap == MFS_U_TANH) ? tanh(x) : x;
    const int J1 = degree + 1;
    double am = coef[degree], av = coef[J1 + degree], dm = 0.0;
    for (int j = degree - 1; j >= 0; --j) {
        if (DERIV) dm = dm * u + am;
        am = am * u + coef[j];
        av = av * u + coef[J1 + j];
    }
    mu = c * x + am;
    var = av;
    dmu = DERIV ? c + dm * ((umap == MFS_U_TANH) ? 1.0 - u * u : 1.0) : 0.0;
}

template <int L, bool EKF>
__global__ void __launch_bounds__(kGfThreads) gf_filter_1d(const GfArgs a) {
    extern __shared__ double gf_lds[];
    constexpr int G = kGfThreads / L;   // replicates per block
    const int tid = threadIdx.x, g = tid / L, l = tid % L;
    const int n = EKF ? 0 : a.n_points;
    const int csz = 2 * (a.degree + 1);
    double* s_xi = gf_lds;
    double* s_w = s_xi + n;
    double* s_coef = s_w + n;
    double* s_lik = s_coef + (a.coef_batched ? G : 1) * csz;
    const int b = blockIdx.x * G + g;
    const bool live = b < a.B;
    const int bb = live ? b : a.B - 1;

    for (int i = tid; i < n; i += kGfThreads) {
        s_xi[i] = a.xi[i];
        s_w[i] = a.w[i];
    }
    if (a.coef_batched) {
        for (int i = l; i < csz; i += L) s_coef[g * csz + i] = a.coef[(size_t)bb * csz + i];
    } else {
        for (int i = tid; i < csz; i += kGfThreads) s_coef[i] = a.coef[i];
    }
    if (a.lik_batched) {
        for (int i = l; i < a.n_lik; i += L) s_lik[g * a.n_lik + i] = a.lik[(size_t)bb * a.n_lik + i];
    } else {
        for (int i = tid; i < a.n_lik; i += kGfThreads) s_lik[i] = a.lik[i];
    }
    __syncthreads();
    const double* coef = s_coef + (a.coef_batched ? g * csz : 0);
    const GfLik lp = gf_load_lik(s_lik + (a.lik_batched ? g * a.n_lik : 0), a.n_lik);
    const int kind = a.lik_kind, degree = a.degree, umap = a.umap;
    const double cx = a.mean_x_coef;
    const double* ys = a.ys + (size_t)bb * a.T;
    const bool store = live && l == 0;
    const double qnan = __builtin_nan("");

    double m = a.m0[a.init_batched ? bb : 0], v = a.P0[a.init_batched ? bb : 0], nell = 0.0;
    int first_nan = -1;
    for (int t = 0; t < a.T; ++t) {
        const double y = ys[t];
        double mp, vp, pred, S, C;
        bool ok = true;
        if (EKF) {
            double var, F;
            gf_trans_1d<true>(coef, degree, umap, cx, m, mp, var, F);
            vp = F * F * v + var;
            const GfMeas q = gf_measure<true>(kind, lp, mp);
            pred = q.h;
            S = q.dh * q.dh * vp + q.xi;
            C = vp * q.dh;
        } else {
            ok = gf_pivot_ok(v);
            const double sd = sqrt(v);
            double s0 = 0.0, s1 = 0.0;
            for (int i = l; i < n; i += L) {
                double mu, var, unused;
                gf_trans_1d<false>(coef, degree, umap, cx, m + sd * s_xi[i], mu, var, unused);
                const double w = s_w[i];
                s0 += w * mu;
                s1 += w * (mu * mu + var);
            }
            mp = group_sum<L>(s0);
            vp = group_sum<L>(s1) - mp * mp;
            ok = ok && gf_pivot_ok(vp);
            const double sdp = sqrt(vp);
            double a0 = 0.0, a1 = 0.0, a2 = 0.0;
            for (int i = l; i < n; i += L) {
                const double x = mp + sdp * s_xi[i];
                const GfMeas q = gf_measure<false>(kind, lp, x);
                const double w = s_w[i];
                a0 += w * q.h;
                a1 += w * (q.h * q.h + q.xi);
                a2 += w * (x * q.h);
            }
            pred = group_sum<L>(a0);
            S = group_sum<L>(a1) - pred * pred;
            C = group_sum<L>(a2) - mp * pred;
        }
        ok = ok && S > 0.0 && finite(S) && finite(y);
        if (ok) {
            const double K = C / S, r = y - pred;
            m = mp + K * r;
            v = vp - K * K * S;
            nell += 0.5 * (r * r / S + log(6.283185307179586476925 * S));
        } else {
            m = qnan;
            v = qnan;
            nell = qnan;
            if (first_nan < 0) first_nan = t;
        }
        if (store) {
            const size_t o = (size_t)b * a.T + t;
            if (a.out_means) a.out_means[o] = m;
            if (a.out_covs) a.out_covs[o] = v;
            a.out_nells[o] = nell;
        }
    }
    if (store && a.out_first_nan) a.out_first_nan[b] = first_nan;
}

// ---------------------------------------------------------------------------------------------------------------
// d = 2
// ---------------------------------------------------------------------------------------------------------------
template <int L, bool EKF>
__global__ void __launch_bounds__(kGfThreads) gf_filter_2d(const GfArgs a) {
    extern __shared__ double gf_lds[];
    constexpr int G = kGfThreads / L;
    const int tid = threadIdx.x, g = tid / L, l = tid % L;
    const int n = EKF ? 0 : a.n_points;
    const int D = a.extent, DD = D * D, csz = 5 * DD;
    double* s_xi = gf_lds;            // [n][2]
    double* s_w = s_xi + 2 * n;
    double* s_coef = s_w + n;         // mu_0, mu_1, S_00, S_01, S_11
    double* s_lik = s_coef + csz;     // [MFS_MAX_LIK] or [G][MFS_MAX_LIK]
    const int b = blockIdx.x * G + g;
    const bool live = b < a.B;
    const int bb = live ? b : a.B - 1;

    for (int i = tid; i < n; i += kGfThreads) {
        s_xi[2 * i] = a.xi[2 * i];
        s_xi[2 * i + 1] = a.xi[2 * i + 1];
        s_w[i] = a.w[i];
    }
    for (int i = tid; i < csz; i += kGfThreads) s_coef[i] = a.coef[i];
    if (a.lik_batched) {
        for (int i = l; i < MFS_MAX_LIK; i += L) s_lik[g * MFS_MAX_LIK + i] = a.lik[(size_t)bb * MFS_MAX_LIK + i];
    } else {
        for (int i = tid; i < MFS_MAX_LIK; i += kGfThreads) s_lik[i] = a.lik[i];
    }
    __syncthreads();
    const GfLik lp = gf_load_lik(s_lik + (a.lik_batched ? g * MFS_MAX_LIK : 0), MFS_MAX_LIK);
    const int kind = a.lik_kind;
    const bool on0 = a.component == 0;   // the state component the measurement reads
    const double* c_m0 = s_coef;
    const double* c_m1 = s_coef + DD;
    const double* c_s00 = s_coef + 2 * DD;
    const double* c_s01 = s_coef + 3 * DD;
    const double* c_s11 = s_coef + 4 * DD;
    const double* ys = a.ys + (size_t)bb * a.T;
    const bool store = live && l == 0;
    const double qnan = __builtin_nan("");

    const double* m0 = a.m0 + (a.init_batched ? (size_t)bb * 2 : 0);
    const double* P0 = a.P0 + (a.init_batched ? (size_t)bb * 4 : 0);
    double m_0 = m0[0], m_1 = m0[1], p00 = P0[0], p01 = P0[2], p11 = P0[3], nell = 0.0;
    int first_nan = -1;
    for (int t = 0; t < a.T; ++t) {
        const double y = ys[t];
        double mp0, mp1, q00, q01, q11, pred, S, C0, C1;
        bool ok = true;
        if (EKF) {
            double f00, f01, f10, f11;
            mp0 = gf_poly2_grad(c_m0, D, m_0, m_1, f00, f01);
            mp1 = gf_poly2_grad(c_m1, D, m_0, m_1, f10, f11);
            // F P F^T + S(m)
            const double t00 = f00 * p00 + f01 * p01, t01 = f00 * p01 + f01 * p11;
            const double t10 = f10 * p00 + f11 * p01, t11 = f10 * p01 + f11 * p11;
            q00 = t00 * f00 + t01 * f01 + gf_poly2(c_s00, D, m_0, m_1);
            q01 = t00 * f10 + t01 * f11 + gf_poly2(c_s01, D, m_0, m_1);
            q11 = t10 * f10 + t11 * f11 + gf_poly2(c_s11, D, m_0, m_1);
            const GfMeas q = gf_measure<true>(kind, lp, on0 ? mp0 : mp1);
            pred = q.h;
            S = q.dh * q.dh * (on0 ? q00 : q11) + q.xi;
            C0 = (on0 ? q00 : q01) * q.dh;
            C1 = (on0 ? q01 : q11) * q.dh;
        } else {
            double l00, l10, l11;
            ok = gf_chol2(p00, p01, p11, l00, l10, l11);
            double s0 = 0.0, s1 = 0.0, s00 = 0.0, s01 = 0.0, s11 = 0.0;
            for (int i = l; i < n; i += L) {
                const double e0 = s_xi[2 * i], e1 = s_xi[2 * i + 1], w = s_w[i];
                const double x0 = m_0 + l00 * e0, x1 = m_1 + (l10 * e0 + l11 * e1);
                const double mu0 = gf_poly2(c_m0, D, x0, x1), mu1 = gf_poly2(c_m1, D, x0, x1);
                s0 += w * mu0;
                s1 += w * mu1;
                s00 += w * (mu0 * mu0 + gf_poly2(c_s00, D, x0, x1));
                s01 += w * (mu0 * mu1 + gf_poly2(c_s01, D, x0, x1));
                s11 += w * (mu1 * mu1 + gf_poly2(c_s11, D, x0, x1));
            }
            mp0 = group_sum<L>(s0);
            mp1 = group_sum<L>(s1);
            q00 = group_sum<L>(s00) - mp0 * mp0;
            q01 = group_sum<L>(s01) - mp0 * mp1;
            q11 = group_sum<L>(s11) - mp1 * mp1;
            const bool okp = gf_chol2(q00, q01, q11, l00, l10, l11);
            ok = ok && okp;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
            for (int i = l; i < n; i += L) {
                const double e0 = s_xi[2 * i], e1 = s_xi[2 * i + 1], w = s_w[i];
                const double x0 = mp0 + l00 * e0, x1 = mp1 + (l10 * e0 + l11 * e1);
                const GfMeas q = gf_measure<false>(kind, lp, on0 ? x0 : x1);
                a0 += w * q.h;
                a1 += w * (q.h * q.h + q.xi);
                a2 += w * (x0 * q.h);
                a3 += w * (x1 * q.h);
            }
            pred = group_sum<L>(a0);
            S = group_sum<L>(a1) - pred * pred;
            C0 = group_sum<L>(a2) - mp0 * pred;
            C1 = group_sum<L>(a3) - mp1 * pred;
        }
        ok = ok && S > 0.0 && finite(S) && finite(y);
        if (ok) {
            const double K0 = C0 / S, K1 = C1 / S, r = y - pred;
            m_0 = mp0 + K0 * r;
            m_1 = mp1 + K1 * r;
            p00 = q00 - K0 * K0 * S;
            p01 = q01 - K0 * K1 * S;
            p11 = q11 - K1 * K1 * S;
            nell += 0.5 * (r * r / S + log(6.283185307179586476925 * S));
        } else {
            m_0 = m_1 = p00 = p01 = p11 = nell = qnan;
            if (first_nan < 0) first_nan = t;
        }
        if (store) {
            const size_t o = (size_t)b * a.T + t;
            if (a.out_means) {
                a.out_means[2 * o] = m_0;
                a.out_means[2 * o + 1] = m_1;
            }
            if (a.out_covs) {
                a.out_covs[4 * o] = p00;
                a.out_covs[4 * o + 1] = p01;
                a.out_covs[4 * o + 2] = p01;
                a.out_covs[4 * o + 3] = p11;
            }
            a.out_nells[o] = nell;
        }
    }
    if (store && a.out_first_nan) a.out_first_nan[b] = first_nan;
}

}  // namespace mfs
