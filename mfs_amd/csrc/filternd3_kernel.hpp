// filternd3_kernel.hpp -- hand-written HIP for gfx950: the N-D moment-filter time-step loop for d = 3 states.
//
// Reference: mfs/multi_dims/filtering.py:33-344 (the three filters), mfs/multi_dims/quadratures.py:120-178
// (moment_quadrature_nd), mfs/multi_dims/moments.py:257-479 (TME operator tables and the Normal closures).
//
// One filter per 256-thread workgroup (4 waves); the time loop runs inside the kernel.  Per half-step:
//   front end   G = m[inds[0]], H_k = m[inds[1 + k]] (s x s, s = C(N + 2, 3) <= 20) gathered into LDS; Cholesky (or the LDL^T
//               completion of mfs/utils.py:495-538 when stable) right-looking with one barrier pair per column; K_k = R^-1 H_k R^-T
//               by two triangular substitutions, one thread per (k, column) with the column in registers; the three symmetric
//               eigensolves by parallel cyclic Jacobi (round-robin pairing: s / 2 disjoint rotations of all three matrices per
//               round, columns then rows, then a sweep-level convergence flag).
//   weights     the rule's s^3 nodes are never listed: a node (i, j, l) is (lambda0_i, lambda1_j, lambda2_l) and its weight the chain
//               W = v0_i[0] C01[i][j] C12[j][l] v2_l[0] with C01 = V0^T V1, C12 = V1^T V2 (quadratures.py:165-170), formed on the fly.
//   node passes every sum of the step is sum_nodes W f(x) for a vector integrand f of Q rows (Q = z for moments, 3..6 for means and
//               scales).  Nodes go through an LDS tile of TILE columns: one thread per node writes its column (moments by a
//               recursion down the graded-lex table, in place), then the workgroup reduces the tile row-wise into one register
//               per (row, column group).  Summation order is fixed, so a replicate's bits do not depend on its batch position.
//   predict     operator tables: E[(X'-c)^n | x] = (x-c)^n + sum_kappa Q_kappa(x) n!/(n-kappa)! (x-c)^(n-kappa), 34 kappa with
//               |kappa| <= 4, evaluated per node (Horner per coefficient block, the block's true extents);
//               Normal closures: the 3-D Stein recursion M(a) = m_k M(a - e_k) + sum_j (a - e_k)_j S_kj M(a - e_k - e_j), k the
//               first nonzero index of a, per node from M(0) = W.
//   update      the likelihood is a product of single-component factors: lik_k(x_k) tabulated on the s eigenvalues of each
//               component, the node value a product of three table entries.  Joint factors (J = 1 instantiations, FilterNd3Joint):
//               kind(y; u(x)) with u = p, sqrt(p), atan2(p, q) or atan2(p, sqrt(q)) of trivariate polynomials, evaluated at the
//               node from its coordinates and multiplied into the node weight in each of the three update passes (recomputed per
//               pass: s^3 values do not fit in LDS at N = 4).  J = 0 instantiations carry none of it.
// A replicate whose rule fails (non-positive pivot, non-finite K) or whose moments turn non-finite is NaN-poisoned from that
// step on; out_first_nan reports the step.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include "../../include/mfs_hip.h"
#include "kernel_args.hpp"   // FilterNd3Args, FilterNd3Joint, nd3_count / nd3_index / nd3_exp / nd3_perm / nd3_kappa_row
#include "likelihood.hpp"    // likelihood_nd, lik_density

namespace mfs {

template <class F, int... I>
__device__ __forceinline__ void nd3_fold(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int E, class F>
__device__ __forceinline__ void nd3_for(F&& f) { nd3_fold(f, std::make_integer_sequence<int, E>{}); }

// LDS layout (doubles) of one workgroup
template <int N>
struct Nd3Tile {
    static constexpr int S = N * (N + 1) * (N + 2) / 6;          // Gram size
    static constexpr int Z = nd3_count(2 * N - 1);                // moments
    static constexpr int SS = S * S;
    static constexpr int NN = S * S * S;                          // tensor nodes
    static constexpr int H = S / 2;                               // rotations per Jacobi round
    static constexpr int TILE = (N == 2) ? 64 : 128;              // node columns per tile (N = 2: s^3 = 64 nodes)
    static constexpr int TS = TILE + 1;                           // row stride of the tile (odd: conflict-free row reads)
    static constexpr int oA = 0;                                  // [3][S][S] H_k -> K_k -> Jacobi iterate
    static constexpr int oV = oA + 3 * SS;                        // [3][S][S] eigenvectors (columns)
    static constexpr int oR = oV + 3 * SS;                        // [S][S] Cholesky factor (lower)
    static constexpr int oC01 = oR + SS;
    static constexpr int oC12 = oC01 + SS;
    static constexpr int oW0 = oC12 + SS;                         // v0_i[0]
    static constexpr int oW2 = oW0 + S;                           // v2_l[0]
    static constexpr int oX = oW2 + S;                            // [3][S] node coordinates per component
    static constexpr int oL = oX + 3 * S;                         // [3][S] likelihood per component
    static constexpr int oMom = oL + 3 * S;                       // [Z] current moments
    static constexpr int oMisc = oMom + Z;                        // mean[3], scale[3], acc[8], eps, tol[3], int flags
    static constexpr int oRot = oMisc + 32;                       // [3][H][8] rotation parameters
    static constexpr int oRed = oRot + 3 * H * 8;                 // [256] reduction / factorisation scratch
    static constexpr int oTile = oRed + 256;                      // [Z][TS]
    static constexpr int kDoubles = oTile + Z * TS;
    static_assert(S % 2 == 0, "round-robin Jacobi pairing needs an even s");
    static_assert(kDoubles * 8 <= 160 * 1024, "LDS budget");
    static_assert(256 / Z >= 2 || Z > 128, "reduction groups");
};
// misc slots
constexpr int kM3Mean = 0, kM3Scale = 3, kM3Acc = 6, kM3Eps = 14, kM3Tol = 15, kM3Flag = 20;   // flags: ints at double slot 20..

// polynomial of one coefficient block at (x0, x1, x2), Horner over the block's true extents
__device__ __forceinline__ double nd3_poly(const double* __restrict__ c, const int D, const int ext, const double x0,
                                           const double x1, const double x2) {
    const int ea = ext & 255, eb = (ext >> 8) & 255, ec = (ext >> 16) & 255;
    double r = 0.0;
    for (int i = ea - 1; i >= 0; --i) {
        double s1 = 0.0;
        for (int j = eb - 1; j >= 0; --j) {
            const double* row = c + (i * D + j) * D;
            double s2 = 0.0;
            for (int k = ec - 1; k >= 0; --k) s2 = fma(s2, x2, row[k]);
            s1 = fma(s1, x1, s2);
        }
        r = fma(r, x0, s1);
    }
    return r;
}

// one joint factor at a node: the link u of p and q, then the kind's density of u (lik_density, likelihood.hpp).
// sqrt of a negative value is NaN; a non-finite u gives NaN, which poisons the replicate through p(y).
__device__ __forceinline__ double nd3_joint_factor(const int kind, const int link, const double* __restrict__ c, const int E,
                                                   const int extp, const int extq, const double par, const double y,
                                                   const double x0, const double x1, const double x2) {
    const double p = nd3_poly(c, E, extp, x0, x1, x2);
    double u = p;
    if (link == MFS_ND3_LINK_SQRT) {
        u = sqrt(p);
    } else if (link != MFS_ND3_LINK_POLY) {
        const double q = nd3_poly(c + E * E * E, E, extq, x0, x1, x2);
        u = atan2(p, (link == MFS_ND3_LINK_ATAN2_SQRT) ? sqrt(q) : q);
    }
    if (!__builtin_isfinite(u)) return __builtin_nan("");
    return lik_density<true>(kind, u, par, y);
}

// The quadrature rule of the moments in LDS (oMom) around the centre / scale in misc (mode): on return the node coordinates
// (oX), the chain factors (oW0, oC01, oC12, oW2).  false (uniform) when the rule does not exist: the replicate is poisoned.
template <int N>
__device__ bool nd3_rule(double* __restrict__ Sm, const int32_t* __restrict__ inds, const int mode, const int stable) {
    using L = Nd3Tile<N>;
    constexpr int S = L::S, SS = L::SS, H = L::H;
    const int tid = threadIdx.x;
    int* flags = reinterpret_cast<int*>(Sm + L::oMisc + kM3Flag);
    // gather G (into R) and H_k (into A_k); inds was checked on the host to be the graded-lex table (entries < z)
    for (int t = tid; t < 4 * SS; t += 256) {
        const double v = Sm[L::oMom + inds[t]];
        Sm[(t < SS) ? L::oR + t : L::oA + (t - SS)] = v;
    }
    if (tid == 0) { flags[0] = 0; flags[1] = 0; }
    __syncthreads();
    if (stable && tid == 0) {          // eps = 1e-8 ||G||_F (mfs/utils.py:525-538)
        double f = 0.0;
        for (int e = 0; e < SS; ++e) f = fma(Sm[L::oR + e], Sm[L::oR + e], f);
        Sm[L::oMisc + kM3Eps] = 1e-8 * sqrt(f);
    }
    // right-looking factorisation: Cholesky, or LDL^T with the unit factor in R and d in oRed[S..2S)
    double* col = Sm + L::oRed;
    for (int j = 0; j < S; ++j) {
        const double piv = Sm[L::oR + j * S + j];
        if (!stable && !(piv > 0.0)) return false;      // not positive definite (NaN included): uniform, every thread read piv
        const double den = stable ? piv : sqrt(piv);
        for (int i = j + 1 + tid; i < S; i += 256) col[i] = Sm[L::oR + i * S + j] / den;
        __syncthreads();
        constexpr int kTri = S * (S + 1) / 2;
        for (int t = tid; t < kTri; t += 256) {          // (i, k), k <= i, of the trailing block j < k <= i < S
            int i = 0;
            while ((i + 1) * (i + 2) / 2 <= t) ++i;
            const int k = t - i * (i + 1) / 2;
            if (k > j) Sm[L::oR + i * S + k] -= stable ? col[i] * col[k] * piv : col[i] * col[k];
        }
        for (int i = j + 1 + tid; i < S; i += 256) { Sm[L::oR + i * S + j] = col[i]; Sm[L::oR + j * S + i] = 0.0; }
        if (tid == 0) { Sm[L::oR + j * S + j] = stable ? 1.0 : den; col[S + j] = piv; }
        __syncthreads();
    }
    if (stable) {                      // R = L diag(d < 0 ? eps : sqrt(d))
        const double eps = Sm[L::oMisc + kM3Eps];
        for (int t = tid; t < SS; t += 256) {
            const int i = t / S, k = t % S;
            const double d = col[S + k];
            if (k <= i) Sm[L::oR + t] *= (d < 0.0) ? eps : sqrt(d);
        }
        __syncthreads();
    }
    // X = R^-1 H_k, one thread per (k, column c) with the column in registers; written back over H_k's column
    if (tid < 3 * S) {
        const int m = tid / S, c = tid % S;
        double* A = Sm + L::oA + m * SS;
        double x[S];
#pragma unroll
        for (int i = 0; i < S; ++i) {
            double v = A[i * S + c];
#pragma unroll
            for (int k = 0; k < i; ++k) v = fma(-Sm[L::oR + i * S + k], x[k], v);
            x[i] = v / Sm[L::oR + i * S + i];
        }
#pragma unroll
        for (int i = 0; i < S; ++i) A[i * S + c] = x[i];
    }
    __syncthreads();
    // K = (R^-1 X^T)^T: row r of K solves R y = (row r of X)
    if (tid < 3 * S) {
        const int m = tid / S, r = tid % S;
        double* A = Sm + L::oA + m * SS;
        double y[S];
#pragma unroll
        for (int i = 0; i < S; ++i) {
            double v = A[r * S + i];
#pragma unroll
            for (int k = 0; k < i; ++k) v = fma(-Sm[L::oR + i * S + k], y[k], v);
            y[i] = v / Sm[L::oR + i * S + i];
        }
#pragma unroll
        for (int i = 0; i < S; ++i) A[r * S + i] = y[i];
    }
    __syncthreads();
    // symmetrise (jax.lax.linalg.eigh symmetrize_input) and check
    for (int t = tid; t < 3 * SS; t += 256) {
        const int m = t / SS, e = t % SS, i = e / S, k = e % S;
        if (i < k) {
            double* A = Sm + L::oA + m * SS;
            const double v = 0.5 * (A[i * S + k] + A[k * S + i]);
            A[i * S + k] = v; A[k * S + i] = v;
            if (!__builtin_isfinite(v)) flags[0] = 1;
        } else if (i == k && !__builtin_isfinite(Sm[L::oA + t])) {
            flags[0] = 1;
        }
    }
    __syncthreads();
    if (flags[0]) return false;
    if (tid < 3) {                     // convergence threshold of the rotations: 1e-18 ||K_k||_F
        double f = 0.0;
        for (int e = 0; e < SS; ++e) f = fma(Sm[L::oA + tid * SS + e], Sm[L::oA + tid * SS + e], f);
        Sm[L::oMisc + kM3Tol + tid] = 1e-18 * sqrt(f);
    }
    for (int t = tid; t < 3 * SS; t += 256) Sm[L::oV + t] = ((t % SS) / S == (t % S)) ? 1.0 : 0.0;
    __syncthreads();
    // parallel cyclic Jacobi on the three matrices
    constexpr int kMaxSweeps = 40;
    for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
        for (int r = 0; r < S - 1; ++r) {
            // rotation parameters (Numerical Recipes' form); pair p of round r by the circle method
            if (tid < 3 * H) {
                const int m = tid / H, p = tid % H;
                int a0 = (p == 0) ? S - 1 : (r + p) % (S - 1), a1 = (p == 0) ? r : (r - p + (S - 1)) % (S - 1);
                const int pp = a0 < a1 ? a0 : a1, qq = a0 < a1 ? a1 : a0;
                const double* A = Sm + L::oA + m * SS;
                const double apq = A[pp * S + qq], app = A[pp * S + pp], aqq = A[qq * S + qq];
                double c = 1.0, s = 0.0, t = 0.0;
                if (fabs(apq) > Sm[L::oMisc + kM3Tol + m]) {
                    const double th = (aqq - app) / (2.0 * apq);
                    t = (fabs(th) > 1e150) ? 0.5 / th : copysign(1.0, th) / (fabs(th) + sqrt(fma(th, th, 1.0)));
                    c = 1.0 / sqrt(fma(t, t, 1.0));
                    s = t * c;
                    flags[1] = 1;
                }
                double* rp = Sm + L::oRot + (m * H + p) * 8;
                rp[0] = (double)pp; rp[1] = (double)qq; rp[2] = c; rp[3] = s; rp[4] = t; rp[5] = apq; rp[6] = app; rp[7] = aqq;
            }
            __syncthreads();
            // columns pp, qq of A_m and V_m
            for (int t = tid; t < 3 * H * S * 2; t += 256) {
                const int w = t / (3 * H * S), u = t % (3 * H * S);
                const int mp = u / S, row = u % S, m = mp / H;
                const double* rp = Sm + L::oRot + mp * 8;
                const int pp = (int)rp[0], qq = (int)rp[1];
                const double c = rp[2], s = rp[3];
                double* M = Sm + (w ? L::oV : L::oA) + m * SS + row * S;
                const double x = M[pp], y = M[qq];
                M[pp] = c * x - s * y;
                M[qq] = s * x + c * y;
            }
            __syncthreads();
            // rows pp, qq of A_m; the 2 x 2 block takes its exact rotated values
            for (int t = tid; t < 3 * H * S; t += 256) {
                const int mp = t / S, cl = t % S, m = mp / H;
                const double* rp = Sm + L::oRot + mp * 8;
                const int pp = (int)rp[0], qq = (int)rp[1];
                const double c = rp[2], s = rp[3], tt = rp[4], apq = rp[5];
                double* A = Sm + L::oA + m * SS;
                if (cl == pp) {
                    A[pp * S + pp] = rp[6] - tt * apq; A[qq * S + pp] = 0.0;
                } else if (cl == qq) {
                    A[pp * S + qq] = 0.0; A[qq * S + qq] = rp[7] + tt * apq;
                } else {
                    const double x = A[pp * S + cl], y = A[qq * S + cl];
                    A[pp * S + cl] = c * x - s * y;
                    A[qq * S + cl] = s * x + c * y;
                }
            }
            __syncthreads();
        }
        const int rotated = flags[1];
        __syncthreads();
        if (tid == 0) flags[1] = 0;
        __syncthreads();
        if (!rotated) break;
    }
    // node coordinates (quadratures.py:175-178) and the chain factors of the weights
    for (int t = tid; t < 3 * S; t += 256) {
        const int m = t / S, i = t % S;
        const double lam = Sm[L::oA + m * SS + i * S + i];
        Sm[L::oX + t] = (mode == MFS_MODE_RAW) ? lam
                      : (mode == MFS_MODE_SCALED) ? fma(lam, Sm[L::oMisc + kM3Scale + m], Sm[L::oMisc + kM3Mean + m])
                                                  : lam + Sm[L::oMisc + kM3Mean + m];
    }
    for (int t = tid; t < 2 * SS + 2 * S; t += 256) {
        if (t < 2 * SS) {
            const int w = t / SS, e = t % SS, i = e / S, k = e % S;
            const double* Va = Sm + L::oV + w * SS;
            const double* Vb = Va + SS;
            double acc = 0.0;
#pragma unroll
            for (int r = 0; r < S; ++r) acc = fma(Va[r * S + i], Vb[r * S + k], acc);
            Sm[(w ? L::oC12 : L::oC01) + e] = acc;
        } else {
            const int u = t - 2 * SS, w = u / S, i = u % S;
            Sm[(w ? L::oW2 : L::oW0) + i] = Sm[L::oV + (w ? 2 * SS : 0) + i];
        }
    }
    __syncthreads();
    return true;
}

// out[q] = sum over the s^3 nodes of the column f writes (rows q < Q); see the header comment.  Every thread calls it.
template <int N, int Q, class F>
__device__ __forceinline__ void nd3_pass(double* __restrict__ Sm, double* __restrict__ out, F&& f) {
    using L = Nd3Tile<N>;
    constexpr int S = L::S, G = 256 / Q;
    static_assert(Q >= 1 && Q <= 256 && Q <= L::Z + 8, "rows");
    const int tid = threadIdx.x, q = tid % Q, g = tid / Q;
    double part = 0.0;
    for (int base = 0; base < L::NN; base += L::TILE) {
        if (tid < L::TILE) {
            double* colp = Sm + L::oTile + tid;
            const int node = base + tid;
            if (node < L::NN) {
                const int i = node / (S * S), j = (node / S) % S, k = node % S;
                const double W = Sm[L::oW0 + i] * Sm[L::oC01 + i * S + j] * Sm[L::oC12 + j * S + k] * Sm[L::oW2 + k];
                f(colp, i, j, k, W, Sm[L::oX + i], Sm[L::oX + S + j], Sm[L::oX + 2 * S + k]);
            } else {
#pragma unroll
                for (int r = 0; r < Q; ++r) colp[r * L::TS] = 0.0;
            }
        }
        __syncthreads();
        if (g < G)
            for (int c = g; c < L::TILE; c += G) part += Sm[L::oTile + q * L::TS + c];
        __syncthreads();
    }
    if (g < G) Sm[L::oRed + g * Q + q] = part;
    __syncthreads();
    if (tid < Q) {
        double s = 0.0;
        for (int gg = 0; gg < G; ++gg) s += Sm[L::oRed + gg * Q + tid];
        out[tid] = s;
    }
    __syncthreads();
}

// column of monomials: col[n] = col[0] * u^n for every n of the table (col[0] already written), ascending
template <int Z>
__device__ __forceinline__ void nd3_monomials(double* __restrict__ colp, const int ts, const double u0, const double u1,
                                              const double u2) {
    nd3_for<Z - 1>([&](auto I) {
        constexpr int i = I + 1;
        constexpr int a = nd3_exp(i, 0), b = nd3_exp(i, 1), c = nd3_exp(i, 2);
        constexpr int k = (a > 0) ? 0 : (b > 0) ? 1 : 2;
        constexpr int src = nd3_index(a - (k == 0), b - (k == 1), c - (k == 2));
        const double u = (k == 0) ? u0 : (k == 1) ? u1 : u2;
        colp[i * ts] = colp[src * ts] * u;
    });
}

template <int N, int TK, int J>
__device__ __forceinline__ void filternd3_body(const FilterNd3Args& a, const FilterNd3Joint& jt) {
    using L = Nd3Tile<N>;
    constexpr int S = L::S, Z = L::Z, TS = L::TS;
    extern __shared__ double Sm[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int mode = a.mode;
    const double* coef = a.coef + (a.coef_batched ? (size_t)b * MFS_ND3_ROWS * a.D * a.D * a.D : 0);
    const double* lik = a.lik + (a.lik_batched ? (size_t)b * a.n_factors * MFS_MAX_LIK : 0);
    const int D = a.D, DDD = D * D * D;
    double* misc = Sm + L::oMisc;
    int* flags = reinterpret_cast<int*>(misc + kM3Flag);

    const double* m0 = a.m0 + (a.m0_batched ? (size_t)b * Z : 0);
    for (int q = tid; q < Z; q += 256) Sm[L::oMom + q] = m0[q];
    if (tid < 3) {
        misc[kM3Mean + tid] = (mode != MFS_MODE_RAW) ? a.mean0[(a.m0_batched ? b * 3 : 0) + tid] : 0.0;
        misc[kM3Scale + tid] = (mode == MFS_MODE_SCALED) ? a.scale0[(a.m0_batched ? b * 3 : 0) + tid] : 1.0;
    }
    if (tid == 0) flags[2] = 0;
    __syncthreads();
    bool poisoned = false;
    int first_nan = -1;
    double nell = 0.0;
    for (int t = 0; t < a.T; ++t) {
        if (!poisoned) {
            // ---- predict (filtering.py:186-190 / :261-263 / :329-330) ----
            bool ok = nd3_rule<N>(Sm, a.inds, mode, a.stable);
            if (ok) {
                if (mode != MFS_MODE_RAW) {
                    constexpr int QM = 6;     // W E[X' | x] (3), W var(X'_k | x) (3, scaled mode)
                    nd3_pass<N, QM>(Sm, misc + kM3Acc, [&](double* colp, int, int, int, double W, double x0, double x1, double x2) {
                        if constexpr (TK == 0) {
                            colp[0] = W * (x0 + nd3_poly(coef + nd3_kappa_row(1, 0, 0) * DDD, D, a.ext[nd3_kappa_row(1, 0, 0)], x0, x1, x2));
                            colp[TS] = W * (x1 + nd3_poly(coef + nd3_kappa_row(0, 1, 0) * DDD, D, a.ext[nd3_kappa_row(0, 1, 0)], x0, x1, x2));
                            colp[2 * TS] = W * (x2 + nd3_poly(coef + nd3_kappa_row(0, 0, 1) * DDD, D, a.ext[nd3_kappa_row(0, 0, 1)], x0, x1, x2));
#pragma unroll
                            for (int k = 0; k < 3; ++k)
                                colp[(3 + k) * TS] = (mode == MFS_MODE_SCALED)
                                    ? W * nd3_poly(coef + (MFS_ND3_TERMS + k) * DDD, D, a.ext[MFS_ND3_TERMS + k], x0, x1, x2) : 0.0;
                        } else {
#pragma unroll
                            for (int k = 0; k < 3; ++k) colp[k * TS] = W * nd3_poly(coef + k * DDD, D, a.ext[k], x0, x1, x2);
                            constexpr int kVar[3] = {3, 6, 8};   // S_00, S_11, S_22
#pragma unroll
                            for (int k = 0; k < 3; ++k)
                                colp[(3 + k) * TS] = (mode == MFS_MODE_SCALED)
                                    ? W * nd3_poly(coef + kVar[k] * DDD, D, a.ext[kVar[k]], x0, x1, x2) : 0.0;
                        }
                    });
                    if (tid < 3) {
                        misc[kM3Mean + tid] = misc[kM3Acc + tid];
                        if (mode == MFS_MODE_SCALED) misc[kM3Scale + tid] = sqrt(misc[kM3Acc + 3 + tid]);
                    }
                    __syncthreads();
                }
                const double c0 = misc[kM3Mean], c1 = misc[kM3Mean + 1], c2 = misc[kM3Mean + 2];   // 0 in raw mode
                nd3_pass<N, Z>(Sm, Sm + L::oMom, [&](double* colp, int, int, int, double W, double x0, double x1, double x2) {
                    if constexpr (TK == 0) {
                        double qv[MFS_ND3_TERMS];
#pragma unroll
                        for (int r = 0; r < MFS_ND3_TERMS; ++r) qv[r] = nd3_poly(coef + r * DDD, D, a.ext[r], x0, x1, x2);
                        colp[0] = W;
                        nd3_monomials<Z>(colp, TS, x0 - c0, x1 - c1, x2 - c2);
                        // in place, highest degree first: the terms of moment n read lower-degree monomials only
                        nd3_for<Z - 1>([&](auto I) {
                            constexpr int i = Z - 1 - I;
                            constexpr int n0 = nd3_exp(i, 0), n1 = nd3_exp(i, 1), n2 = nd3_exp(i, 2);
                            double v = colp[i * TS];
                            nd3_for<MFS_ND3_TERMS>([&](auto R) {
                                constexpr int k0 = nd3_exp(R + 1, 0), k1 = nd3_exp(R + 1, 1), k2 = nd3_exp(R + 1, 2);
                                if constexpr (k0 <= n0 && k1 <= n1 && k2 <= n2) {
                                    constexpr double ff = (double)(nd3_perm(n0, k0) * nd3_perm(n1, k1) * nd3_perm(n2, k2));
                                    v = fma(qv[R] * ff, colp[nd3_index(n0 - k0, n1 - k1, n2 - k2) * TS], v);
                                }
                            });
                            colp[i * TS] = v;
                        });
                    } else {
                        const double m[3] = {nd3_poly(coef, D, a.ext[0], x0, x1, x2) - c0,
                                             nd3_poly(coef + DDD, D, a.ext[1], x0, x1, x2) - c1,
                                             nd3_poly(coef + 2 * DDD, D, a.ext[2], x0, x1, x2) - c2};
                        double sv[6];
#pragma unroll
                        for (int r = 0; r < 6; ++r) sv[r] = nd3_poly(coef + (3 + r) * DDD, D, a.ext[3 + r], x0, x1, x2);
                        colp[0] = W;
                        nd3_for<Z - 1>([&](auto I) {
                            constexpr int i = I + 1;
                            constexpr int n0 = nd3_exp(i, 0), n1 = nd3_exp(i, 1), n2 = nd3_exp(i, 2);
                            constexpr int k = (n0 > 0) ? 0 : (n1 > 0) ? 1 : 2;
                            constexpr int b0 = n0 - (k == 0), b1 = n1 - (k == 1), b2 = n2 - (k == 2);   // beta = alpha - e_k
                            // S_kj at sv: (0,0)=0 (0,1)=1 (0,2)=2 (1,1)=3 (1,2)=4 (2,2)=5
                            constexpr int s0 = (k == 0) ? 0 : (k == 1) ? 1 : 2;
                            constexpr int s1 = (k == 0) ? 1 : (k == 1) ? 3 : 4;
                            constexpr int s2 = (k == 0) ? 2 : (k == 1) ? 4 : 5;
                            double v = m[k] * colp[nd3_index(b0, b1, b2) * TS];
                            if constexpr (b0 > 0) v = fma((double)b0 * sv[s0], colp[nd3_index(b0 - 1, b1, b2) * TS], v);
                            if constexpr (b1 > 0) v = fma((double)b1 * sv[s1], colp[nd3_index(b0, b1 - 1, b2) * TS], v);
                            if constexpr (b2 > 0) v = fma((double)b2 * sv[s2], colp[nd3_index(b0, b1, b2 - 1) * TS], v);
                            colp[i * TS] = v;
                        });
                    }
                });
                if (mode == MFS_MODE_SCALED) {
                    const double s0 = misc[kM3Scale], s1 = misc[kM3Scale + 1], s2 = misc[kM3Scale + 2];
                    for (int q = tid; q < Z; q += 256) {
                        double p = 1.0;
                        for (int e = nd3_exp(q, 0); e > 0; --e) p *= s0;
                        for (int e = nd3_exp(q, 1); e > 0; --e) p *= s1;
                        for (int e = nd3_exp(q, 2); e > 0; --e) p *= s2;
                        Sm[L::oMom + q] /= p;
                    }
                    __syncthreads();
                }
                // ---- update (filtering.py:192-204 / :265-277 / :332-341) ----
                ok = nd3_rule<N>(Sm, a.inds, mode, a.stable);
            }
            if (ok) {
                for (int u = tid; u < 3 * S; u += 256) {
                    const int k = u / S;
                    const double x = Sm[L::oX + u];
                    double l = 1.0;
                    for (int f = 0; f < a.n_factors; ++f)
                        if (a.fac_comp[f] == k)
                            l *= likelihood_nd(a.fac_kind[f], lik + f * MFS_MAX_LIK,
                                               a.ys[((size_t)b * a.T + t) * a.ny + a.fac_ycol[f]], x);
                    Sm[L::oL + u] = l;
                }
                __syncthreads();
                // joint factors: measurements and parameters of this step are uniform; the node value is recomputed in each pass
                double jy[MFS_ND3_MAX_JOINT], jpar[MFS_ND3_MAX_JOINT];
                const double* jcoef = nullptr;
                if constexpr (J) {
                    jcoef = jt.coef + (jt.batched ? (size_t)b * jt.n * 2 * jt.E * jt.E * jt.E : 0);
#pragma unroll
                    for (int f = 0; f < MFS_ND3_MAX_JOINT; ++f) {
                        jy[f] = (f < jt.n) ? a.ys[((size_t)b * a.T + t) * a.ny + jt.ycol[f]] : 0.0;
                        jpar[f] = (f < jt.n) ? jt.par[(jt.batched ? (size_t)b * jt.n : 0) + f] : 1.0;
                    }
                }
                auto node_lik = [&](int i, int j, int k, double x0, double x1, double x2) {
                    double l = Sm[L::oL + i] * Sm[L::oL + S + j] * Sm[L::oL + 2 * S + k];
                    if constexpr (J) {
#pragma unroll
                        for (int f = 0; f < MFS_ND3_MAX_JOINT; ++f)
                            if (f < jt.n)
                                l *= nd3_joint_factor(jt.kind[f], jt.link[f], jcoef + f * 2 * jt.E * jt.E * jt.E, jt.E, jt.ext[f][0],
                                                      jt.ext[f][1], jpar[f], jy[f], x0, x1, x2);
                    }
                    return l;
                };
                nd3_pass<N, 4>(Sm, misc + kM3Acc, [&](double* colp, int i, int j, int k, double W, double x0, double x1, double x2) {
                    const double wl = W * node_lik(i, j, k, x0, x1, x2);
                    colp[0] = wl; colp[TS] = wl * x0; colp[2 * TS] = wl * x1; colp[3 * TS] = wl * x2;
                });
                const double pdf = misc[kM3Acc];
                const double mu0 = misc[kM3Acc + 1] / pdf, mu1 = misc[kM3Acc + 2] / pdf, mu2 = misc[kM3Acc + 3] / pdf;
                double sc0 = 1.0, sc1 = 1.0, sc2 = 1.0;
                if (mode == MFS_MODE_SCALED) {
                    nd3_pass<N, 3>(Sm, misc + kM3Acc + 4, [&](double* colp, int i, int j, int k, double W, double x0, double x1, double x2) {
                        const double wl = W * node_lik(i, j, k, x0, x1, x2);
                        colp[0] = wl * (x0 - mu0) * (x0 - mu0);
                        colp[TS] = wl * (x1 - mu1) * (x1 - mu1);
                        colp[2 * TS] = wl * (x2 - mu2) * (x2 - mu2);
                    });
                    sc0 = sqrt(misc[kM3Acc + 4] / pdf); sc1 = sqrt(misc[kM3Acc + 5] / pdf); sc2 = sqrt(misc[kM3Acc + 6] / pdf);
                }
                const bool raw = (mode == MFS_MODE_RAW);
                const double c0 = raw ? 0.0 : mu0, c1 = raw ? 0.0 : mu1, c2 = raw ? 0.0 : mu2;
                nd3_pass<N, Z>(Sm, Sm + L::oMom, [&](double* colp, int i, int j, int k, double W, double x0, double x1, double x2) {
                    colp[0] = W * node_lik(i, j, k, x0, x1, x2);
                    nd3_monomials<Z>(colp, TS, (x0 - c0) / sc0, (x1 - c1) / sc1, (x2 - c2) / sc2);
                });
                for (int q = tid; q < Z; q += 256) {
                    const double v = Sm[L::oMom + q] / pdf;
                    Sm[L::oMom + q] = v;
                    if (!__builtin_isfinite(v)) flags[2] = 1;
                }
                if (tid < 3) {      // (raw mode keeps the centre at 0: the next prediction is about the origin)
                    misc[kM3Mean + tid] = raw ? 0.0 : (tid == 0) ? mu0 : (tid == 1) ? mu1 : mu2;
                    misc[kM3Scale + tid] = (tid == 0) ? sc0 : (tid == 1) ? sc1 : sc2;
                }
                nell -= log(pdf);
                if (!__builtin_isfinite(mu0) || !__builtin_isfinite(mu1) || !__builtin_isfinite(mu2) ||
                    !__builtin_isfinite(sc0) || !__builtin_isfinite(sc1) || !__builtin_isfinite(sc2)) ok = false;
                __syncthreads();
                if (flags[2]) ok = false;
                __syncthreads();
                if (tid == 0) flags[2] = 0;
            }
            if (!ok) poisoned = true;
            if (first_nan < 0 && (poisoned || !__builtin_isfinite(nell))) first_nan = t;
        }
        // ---- outputs of step t ----
        const double nan = __builtin_nan("");
        if (a.out_mom) {
            double* o = a.out_mom + ((size_t)b * a.T + t) * Z;
            for (int q = tid; q < Z; q += 256) o[q] = poisoned ? nan : Sm[L::oMom + q];
        }
        if (tid < 3) {
            if (a.out_mean) a.out_mean[((size_t)b * a.T + t) * 3 + tid] = poisoned ? nan : misc[kM3Mean + tid];
            if (a.out_scale) a.out_scale[((size_t)b * a.T + t) * 3 + tid] = poisoned ? nan : misc[kM3Scale + tid];
        }
        __syncthreads();
    }
    if (tid == 0) {
        a.out_nell[b] = poisoned ? __builtin_nan("") : nell;
        if (a.out_first_nan) a.out_first_nan[b] = first_nan;
    }
}

template <int N, int TK>
__global__ __launch_bounds__(256, 1) void filternd3_kernel(const FilterNd3Args a) {
    filternd3_body<N, TK, 0>(a, FilterNd3Joint{});
}

// the same step loop with joint likelihood factors in the update
template <int N, int TK>
__global__ __launch_bounds__(256, 1) void filternd3_joint_kernel(const FilterNd3Args a, const FilterNd3Joint jt) {
    filternd3_body<N, TK, 1>(a, jt);
}

}  // namespace mfs
