// filter1d_partner.hpp -- partner-wave variant of the fixed-traits specialised one-wave builds of the fast 1-D kernel
// (filter1d_fast.hpp: SPEC, StepTraits), for the orders with 16 lanes per filter (N = 14, 15).
//
// The one-wave builds run T x (the latency of one step of one wave).  About a fifth of a step is a side branch whose only
// feedback into the next step is a flag: the posterior moments sum wl dx^n / p_y (output store, chunk carry, finite check and
// the pivots-only Hankel elimination that decides the poisoning) and nell -= log p_y.  The next predict half needs only the
// atoms (dx, wl / p_y) and the mean.  Here that branch runs on a second wave:
//
//   * 512-thread workgroups, one per compute unit.  Waves 0..3 are MAIN waves, four filters each in the lane layout of the
//     one-wave builds; wave w + 4 is the PARTNER of wave w and serves the same four filters with the same lane layout.  A
//     workgroup of eight waves puts waves w and w + 4 on one SIMD; the prologue checks that with HW_REG_HW_ID and counts
//     the workgroups it checked and those where it did not hold (g_partner_placement).  Nothing but speed depends on the placement.
//   * Step t, main wave: predict half from the atoms (no elimination), update half up to wl, p_y, 1 / p_y, mean, dx.  It
//     writes dx, wl, 1 / p_y, p_y per lane and its own bad bit (predicted moments, mean) into exchange slot t & 1, executes
//     the step's barrier and issues the read of the partner's flags of round t - 1.  It does not wait for that word there:
//     it keeps the mean of step t in a register, starts step t + 1 with `dead` as it was, and acts on the word -- update
//     `dead`, poison mean and scale, store the mean of step t, NaN if flagged -- behind the column sums of the predict half of
//     step t + 1, the first place of a step that waits for LDS anyway (after the loop for the last step, before the carry).
//   * Round t, partner wave, after barrier t: reads slot t & 1, forms wl dx^n, reduces, multiplies by 1 / p_y, stores the
//     step's moments, accumulates nell, runs the pivots-only elimination on the posterior moments and publishes two bits per
//     filter in flag slot t & 1: "dead after step t" (a moment, the mean or nell of step t was not finite, or the filter was
//     dead before) and "a pivot of the posterior Hankel matrix of step t was not > 0".
//   * The main wave therefore runs at most one step and one predict half ahead of the flag that governs it: it reads the
//     flags of round t - 1 after barrier t and acts on them before it stores anything of step t and before it writes the
//     exchange slot or its bad bit of step t + 1.  Either bit makes the mean of step t NaN and the filter dead, which is what
//     the NaN propagation through the predict half does in the one-wave builds; the partner, which computed the bits,
//     NaN-fills the moments and nell of step t and sets first_nan (pivot bit: t; dead bit: already set at t - 1).  A filter
//     flagged in round t - 1 has by then run the predict half of step t + 1 into its own tile and registers that are
//     overwritten with NaN; it never enters the update half (the eigenvalue loop sees no such filter), hands nothing over
//     and stores nothing but NaN means.
//   * Both slots are double buffers: a slot written before barrier t is read between barriers t and t + 1 and written again
//     only after barrier t + 1.  The late flag keeps that: the word of round t - 1 is written before barrier t; the main
//     wave's read of it is ISSUED right after barrier t, as before, and LDS serves a wave's accesses in order, so the access
//     happens before everything the main wave does in step t + 1 and has completed by the `s_waitcnt lgkmcnt(0)` of barrier
//     t + 1 at the latest; the partner writes that word again only after barrier t + 1.  Only the wait for the register moved.
//
// BARRIERS.  Every wave of the workgroup executes two barriers in the prologue and exactly one per time step: the two role
// bodies below each contain a single `for (t = a.t_begin; t < a.t_end; ++t)` loop without break, continue or return, with
// one partner_barrier() at the top level of the body.  Whether a filter is live, dead or absent (b >= B) only changes what
// the lanes do between the barriers; no lane leaves the kernel early.  There is no spin or poll loop.
//
// Every floating-point operation that feeds an output is the one-wave build's, in its order: the statements of the two halves
// are those of filter1d_fast_kernel for a fixed-traits build, split between the roles, and quadrature_fast is called as it is
// there (the partner's call keeps only the pivots, as the predict half of the one-wave builds does); the SL bits this variant
// adds to its calls (kSlFreezeX, kSlPivMin) drop selects and compares whose results nothing reads, no arithmetic.
// First step of a run (no atoms): the main wave runs the cold full rule on the moments it loads, as the one-wave builds do.
// Start of a chunk: the partner eliminates the carried moments before the first barrier (the flag of step t_begin).
// MFS_PREDICT_RULE=recompute keeps the one-wave launcher (capi.hip).
#pragma once
#include "filter1d_fast.hpp"

namespace mfs {

// leave-one-out switch (Makefile: PARTNERFLAGS), against the full variant: MFS_PARTNER_AB_LOGPY 1 = nell -= log p_y stays on
// the main wave.  (No s_setprio for the main waves: it measured slower.  Both measurements: DESIGN.md section 6.)
#ifndef MFS_PARTNER_AB_LOGPY
#define MFS_PARTNER_AB_LOGPY 0
#endif
// the step-boundary changes of the main wave, one switch each (0 = the shipped code, 1 = the code it replaced):
//   MFS_PARTNER_AB_FLAGLATE   the partner's flags are consumed inside the next step (1: waited for right behind the barrier)
//   MFS_PARTNER_AB_FREEZE     the eigenvalue loop freezes only x of a converged lane (1: lo, hi and prev_step as well)
//   MFS_PARTNER_AB_PIVMIN     the poison flag from a running minimum of the pivots (1: one compare per pivot)
#ifndef MFS_PARTNER_AB_FLAGLATE
#define MFS_PARTNER_AB_FLAGLATE 0
#endif
#ifndef MFS_PARTNER_AB_FREEZE
#define MFS_PARTNER_AB_FREEZE 0
#endif
#ifndef MFS_PARTNER_AB_PIVMIN
#define MFS_PARTNER_AB_PIVMIN 0
#endif

constexpr int kPartnerMainWaves = 4;                       // main waves per workgroup = SIMDs per compute unit
constexpr int kPartnerThreads = 2 * kPartnerMainWaves * 64;

// [0] workgroups whose placement the prologue checked, [1] those whose waves w and w + 4 were not on one SIMD, summed over the
// launches of the process.  One copy per translation unit that includes this header (the library is built without relocatable
// device code), hence static; every unit registers a reader of its copy and capi.hip adds them up (registry.hpp).
static __device__ unsigned long long g_partner_placement[2];

// the partner's LDS per filter, behind the main waves' tiles (FastTile, as in the one-wave builds)
template <int N, int G>
struct PartnerTile {
    using L = FastTile<N, G>;
    static constexpr int oMom = 0;                         // [2N] posterior moments (Hankel source of the poison elimination)
    static constexpr int oTab = L::M2;                     // [G][2N + 1] per-lane contributions wl dx^n
    static constexpr int oXch = oTab + G * L::TLD;         // [2][4][G] exchange slots: dx, wl, 1 / p_y, p_y of every lane
    static constexpr int oFlag = oXch + 2 * 4 * G;         // ints [0..1]: partner -> main flags, [2..3]: main -> partner bad bit
    static constexpr int kDoubles = oFlag + 2;
    static_assert((kDoubles & 1) == 0, "tiles stay 16-byte aligned");
};
constexpr int kPartnerFlagDead = 1, kPartnerFlagPivot = 2;

// The step's barrier.  s_waitcnt lgkmcnt(0): this wave's LDS writes (exchange slot or flags) have completed; the memory
// clobber keeps the compiler from moving or caching LDS accesses across it.
__device__ __forceinline__ void partner_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <int N, int G, int SPEC, class TR>
__global__ __launch_bounds__(kPartnerThreads, 2) void filter1d_partner_kernel(const Filter1dArgs a, const int lds_doubles) {
    static_assert(G == 16 && N + 1 <= G, "orders with 16 lanes per filter");
    static_assert(TR::fixed && TR::mode == MFS_MODE_CENTRAL, "fixed step traits, central mode");
    static_assert(SPEC == -1 || SPEC == 6, "table shapes with a fixed-traits build");
    using L = FastTile<N, G>;
    using P = PartnerTile<N, G>;
    constexpr int M2 = L::M2, TLD = L::TLD;
    constexpr int FPW = 64 / G, FPB = kPartnerMainWaves * FPW;
    constexpr bool kLogMain = (MFS_PARTNER_AB_LOGPY != 0);
    constexpr bool kFlagLate = (MFS_PARTNER_AB_FLAGLATE == 0);
    constexpr int kSlPivots = (MFS_PARTNER_AB_PIVMIN == 0) ? kSlPivMin : 0;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    // (the wave number as a scalar: the split into roles is a scalar branch, and a wave never walks through the other role's
    //  loop -- and its barriers -- with an empty EXEC mask)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool is_main = wave < kPartnerMainWaves;
    const int grp = lane / G, l = lane - grp * G;
    const int slot = (wave & (kPartnerMainWaves - 1)) * FPW + grp;
    const int b = blockIdx.x * FPB + slot;
    const bool has = b < a.B;                  // an absent filter is a dead one whose stores are switched off
    double* S = smem + (size_t)slot * lds_doubles;
    double* PS = smem + (size_t)FPB * lds_doubles + (size_t)slot * P::kDoubles;
    double* xch = PS + P::oXch;
    int* flags = reinterpret_cast<int*>(PS + P::oFlag);
    const double qnan = __builtin_nan("");
    const bool node = (l < N);

    {   // placement: waves w and w + 4 on one SIMD?  (eight ints at the head of the first exchange slot, not in use yet)
        int* simd = reinterpret_cast<int*>(smem + (size_t)FPB * lds_doubles + P::oXch);
        unsigned hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        if (lane == 0) simd[wave] = (int)((hw >> 4) & 3u);
        __syncthreads();
        if (threadIdx.x == 0) {
            bool same = true;
            for (int w = 0; w < kPartnerMainWaves; ++w) same &= simd[w] == simd[w + kPartnerMainWaves];
            atomicAdd(&g_partner_placement[0], 1ull);
            if (!same) atomicAdd(&g_partner_placement[1], 1ull);
        }
        // (the words belong to an exchange slot: thread 0 has read them before a main wave writes its first hand-over)
        __syncthreads();
    }

    if (is_main) {
        // =============================================================================================================
        // main wave
        // =============================================================================================================
        double* mom = S + L::oMom;
        double* TAB = S + L::oTab;
        const double* coef = S + L::oCoef;
        const double* lp = S + L::oLik;
        double* lfac = S + L::oLfac;
        const int J1 = a.degree + 1;
        if (has) {   // stage the model tables
            const double* src = a.coef + (a.coef_batched ? (size_t)b * a.n_rows * J1 : 0);
            for (int e = l; e < ((a.degree + 4) & ~3) * kCoefRows; e += G) {
                const int j = e / kCoefRows, r = e - j * kCoefRows;
                int sr = r;
                if (a.trans_kind == MFS_TRANS_OPERATOR) sr = (r == MFS_MAX_TERMS) ? a.n_terms : (r < a.n_terms) ? r : a.n_rows;
                S[L::oCoef + e] = (sr < a.n_rows && j < J1) ? src[sr * J1 + j] : 0.0;
            }
            const double* ls = a.lik + (a.lik_batched ? (size_t)b * a.n_lik : 0);
            for (int e = l; e < MFS_MAX_LIK; e += G) S[L::oLik + e] = (e < a.n_lik) ? ls[e] : 0.0;
            if (TR::lik == MFS_LIK_POISSON_SOFTPLUS)
                for (int e = l; e <= kLfacMax; e += G) lfac[e] = log_factorial((double)e);
        }
        double mean = 0.0, scale = 1.0, nell = 0.0;
        int first_nan = -1;
        double gA = qnan, gW = 0.0;
        bool have_atoms = false;
        if (has) {
            if (a.t_begin == 0) {
                const double* src = a.m0 + (a.m0_batched ? (size_t)b * M2 : 0);
                for (int n = l; n < M2; n += G) mom[n] = src[n];
                mean = a.mean0[a.m0_batched ? b : 0];
            } else {
                if (!a.c_lam) for (int n = l; n < M2; n += G) mom[n] = a.c_mom[(size_t)b * M2 + n];   // (no atoms: the cold rule)
                mean = a.c_mean[b];
                scale = a.c_scale[b];
                if constexpr (kLogMain) nell = a.c_nell[b];
                first_nan = a.c_first_nan[b];
                if (a.c_lam) {
                    gA = a.c_lam[((size_t)b * 2 + 0) * G + l];
                    gW = a.c_lam[((size_t)b * 2 + 1) * G + l];
                    have_atoms = true;
                }
            }
        }
        wave_sync();
        constexpr int SR = (SPEC > 0) ? SPEC + 1 : 2;
        constexpr int kVarReg = (SPEC > 0) ? SPEC : -1;
        double tabr[kSpecTop][SR];
        LikRegs lpr;
        // (an absent filter reads whatever its tile holds: nothing of it is ever stored)
#pragma unroll
        for (int q = 0; q < kSpecTop; ++q)
#pragma unroll
            for (int r = 0; r < SR; ++r) tabr[q][r] = coef[q * kCoefRows + ((r == kVarReg) ? MFS_MAX_TERMS : r)];
#pragma unroll
        for (int e = 0; e < MFS_MAX_LIK; ++e) lpr.v[e] = lp[e];
        const bool st_mean = has && a.out_mean && (l == 0);
        size_t o_mean = (size_t)b * a.T + a.t_begin;
        const double* yrow = a.ys + (size_t)b * a.T;
        bool dead = !has || (first_nan >= 0);
        asm volatile("" : "+v"(mean), "+v"(scale), "+v"(nell), "+v"(gA), "+v"(gW), "+v"(first_nan));   // the carry waits, in front of the loop
        double ywin = 0.0;
        constexpr int kSlUpdate = kSlEigLoop | ((MFS_PARTNER_AB_FREEZE == 0) ? kSlFreezeX : 0) | kSlPivots;
        constexpr int trans_kind = (SPEC > 0) ? MFS_TRANS_OPERATOR : MFS_TRANS_GAUSSIAN;
        // the late flag (kFlagLate): the flag word read behind barrier t and the mean of step t, both settled inside step t + 1
        int fl_prev = 0;
        double mean_prev = 0.0, nell_next = nell;
        const auto settle = [&]() __attribute__((always_inline)) {
            if (dead || fl_prev != 0) {
                dead = true;
                mean = qnan; scale = qnan; mean_prev = qnan;
                if constexpr (kLogMain) nell = qnan;
            } else {
                if constexpr (kLogMain) nell = nell_next;
            }
            if (st_mean) a.out_mean[o_mean] = mean_prev;
            o_mean += 1;
        };

        for (int t = a.t_begin; t < a.t_end; ++t) {
            constexpr int YW = 16;
            const int tw = (t - a.t_begin) & (YW - 1);
            if (tw == 0) {
                const double ld = (has && t + (l & (YW - 1)) < a.t_end) ? yrow[t + (l & (YW - 1))] : 0.0;
                asm volatile("v_mov_b64 %0, %1" : "=v"(ywin) : "v"(ld));
            }
            const double y = __shfl(ywin, tw, YW);
            double* xs = xch + (t & 1) * 4 * G;
            if constexpr (!kFlagLate) nell_next = nell;
            int bad = 0;
            double gB = qnan;
            if (!dead) {
                // ---- predict half (filter1d_fast_kernel, half 0)
                auto predict = [&](const auto atoms_ok) __attribute__((always_inline)) {
                    double x, w;
                    double lam_io = gA;
                    if constexpr (decltype(atoms_ok)::value) {
                        // the rule is the posterior's own atoms; the elimination that decides the poisoning runs on the partner
                        x = node ? fma(scale, lam_io, mean) : mean;
                        w = node ? gW : 0.0;
                    } else {
                        quadrature_fast<N, G, false>(mom, l, grp, mean, scale, x, w, lam_io, false, false, gW, S, a.stable);
                    }
                    gB = lam_io;
                    const double u = (TR::umap == MFS_U_TANH) ? fast_tanh(x) : x;
                    double c = 0.0, inv_sc = 1.0;
                    double rows[MFS_MAX_TERMS + 1];
                    {
                        double live[SR];
                        horner_regs<kSpecTop, SR>(tabr, u, live);
#pragma unroll
                        for (int r = 0; r <= MFS_MAX_TERMS; ++r) rows[r] = 0.0;
#pragma unroll
                        for (int r = 0; r < SR; ++r) rows[(r == kVarReg) ? MFS_MAX_TERMS : r] = live[r];
                    }
                    double mu, var;
                    if (trans_kind == MFS_TRANS_OPERATOR) {
                        mu = x + rows[0];
                        var = rows[MFS_MAX_TERMS];
                    } else {
                        mu = fma(a.mean_x_coef, x, rows[0]);
                        var = rows[1];
                    }
                    mean = gsum<G>(w * mu);
                    c = mean;
                    double* row = TAB + l * TLD;
                    if (trans_kind == MFS_TRANS_OPERATOR) {
                        operator_moments<(SPEC > 0) ? SPEC : 2, M2>(rows, x - c, w, inv_sc, node, row);
                    } else {
                        const double ms = (mu - c) * inv_sc, vs = var * inv_sc * inv_sc;
                        double f2 = w, f1 = w * ms, vn = vs;
                        row[0] = f2;
                        row[1] = f1;
#pragma unroll
                        for (int n = 2; n < M2; ++n) {
                            const double f = fma(ms, f1, vn * f2);
                            row[n] = f;
                            vn += vs;
                            f2 = f1;
                            f1 = f;
                        }
                    }
                    wave_sync();
                    {   // column sums of the contribution table -> predicted moments
                        const int n0 = l, n1 = l + G;
                        const bool has0 = n0 < M2, has1 = n1 < M2;
                        const double* t0 = TAB + (has0 ? n0 : 0);
                        const double* t1 = TAB + (has1 ? n1 : 0);
                        double c0[N], c1[N];
#pragma unroll
                        for (int i = 0; i < N; ++i) { c0[i] = t0[i * TLD]; c1[i] = t1[i * TLD]; }
                        __builtin_amdgcn_sched_barrier(0);
                        double s0[3] = {0.0, 0.0, 0.0}, s1[3] = {0.0, 0.0, 0.0};
#pragma unroll
                        for (int i = 0; i < N; ++i) { s0[i % 3] += c0[i]; s1[i % 3] += c1[i]; }
                        const double acc0 = (s0[0] + s0[1]) + s0[2], acc1 = (s1[0] + s1[1]) + s1[2];
                        if (has0) { mom[n0] = acc0; bad |= !finite(acc0); }
                        if (has1) { mom[n1] = acc1; bad |= !finite(acc1); }
                    }
                    wave_sync();
                };
                if (have_atoms) predict(std::true_type{});
                else predict(std::false_type{});   // the first step of a run
            }
            // The flags of round t - 1 and the mean of step t - 1.  The column sums above are the first thing of a step that
            // waits for LDS (the table writes before them only issue), so the flag word, read behind the barrier before any of
            // that, has arrived and this costs no wait of its own; a wait placed earlier would stand behind the table writes,
            // because the LDS counter only counts down in order.  Nothing of step t has been handed over or stored yet: a filter
            // that turns out dead here has computed one predict half for nothing, into its own tile, and stops.
            if constexpr (kFlagLate) { if (t > a.t_begin) settle(); }
            if (!dead) {
                {   // ---- update half (half 1) up to the atoms
                    double x, w;
                    double lam_io = gB;
                    quadrature_fast<N, G, false, kSlUpdate>(mom, l, grp, mean, scale, x, w, lam_io, true, false, gW, S, a.stable);
                    double c = 0.0, inv_sc = 1.0, py = 1.0, ipy = 1.0;
                    const double wl = node ? w * likelihood_sel<true>(TR::lik, lpr, lp, lfac, y, x) : 0.0;
                    py = gsum<G>(wl);
                    ipy = rcp_nr(py);
                    mean = gsum<G>(wl * x) * ipy;
                    c = mean;
                    double dx;
                    {
#pragma clang fp contract(off)
                        dx = (x - c) * inv_sc;
                    }
                    {
                        const double last = bcast<G, N - 1>(dx);
                        gA = node ? dx : last;
                        gW = wl * ipy;
                        have_atoms = true;
                    }
                    if constexpr (kLogMain) {
                        nell_next = nell - fast_log(py);
                        bad |= (int)!finite(nell_next);
                    }
                    bad |= (int)(!finite(mean) || !finite(scale));
                    // hand-over to the partner: slot t & 1
                    xs[0 * G + l] = dx;
                    xs[1 * G + l] = wl;
                    xs[2 * G + l] = ipy;
                    xs[3 * G + l] = py;
                    flags[2 + (t & 1)] = gany<G>(bad != 0, grp) ? 1 : 0;   // (every lane of the group writes the same word)
                }
            }
            partner_barrier();
            // the partner's flags of round t - 1 (the opening of a launch for t = t_begin): read here, before the partner can
            // write the word again, and -- kFlagLate -- waited for and acted on inside step t + 1, or behind the loop
            fl_prev = flags[(t + 1) & 1];
            mean_prev = mean;
            if constexpr (!kFlagLate) settle();
        }
        if constexpr (kFlagLate) { if (a.t_end > a.t_begin) settle(); }   // the last step's mean, before the carry is written
        if (has) {
            if (a.t_end >= a.T) {
                if constexpr (kLogMain) { if (l == 0) a.out_nell[b] = nell; }
            } else {
                if (a.c_lam) { a.c_lam[((size_t)b * 2 + 0) * G + l] = gA; a.c_lam[((size_t)b * 2 + 1) * G + l] = gW; }
                if (l == 0) {
                    a.c_mean[b] = mean; a.c_scale[b] = scale;
                    if constexpr (kLogMain) a.c_nell[b] = nell;
                }
            }
        }
    } else {
        // =============================================================================================================
        // partner wave
        // =============================================================================================================
        double* pmom = PS + P::oMom;
        double* PTAB = PS + P::oTab;
        double nell = 0.0;
        int first_nan = -1;
        bool pivot_prev = false;      // a pivot of the posterior Hankel matrix of the step before was not > 0
        double xd, wd, lamd = qnan;   // (quadrature_fast's outputs: unused, the call keeps only the pivots)
        if (has && a.t_begin != 0) {
            for (int n = l; n < M2; n += G) pmom[n] = a.c_mom[(size_t)b * M2 + n];
            if constexpr (!kLogMain) nell = a.c_nell[b];
            first_nan = a.c_first_nan[b];
        }
        wave_sync();
        bool dead = !has || (first_nan >= 0);
        if (!dead && a.t_begin != 0)   // the flag of step t_begin: the elimination the one-wave builds run in its predict half
            pivot_prev = quadrature_fast<N, G, false, kSlPivots>(pmom, l, grp, 0.0, 1.0, xd, wd, lamd, false, true, 0.0, PS, 0);
        flags[(a.t_begin + 1) & 1] = (dead ? kPartnerFlagDead : 0) | (pivot_prev ? kPartnerFlagPivot : 0);
        const bool st_m0 = has && a.out_mom && l < M2, st_m1 = has && a.out_mom && l + G < M2;
        size_t o_mom = ((size_t)b * a.T + a.t_begin) * M2 + l;

        for (int t = a.t_begin; t < a.t_end; ++t) {
            partner_barrier();
            const double* xs = xch + (t & 1) * 4 * G;
            double out0 = qnan, out1 = qnan;
            if (!dead && !pivot_prev) {
                int bad = flags[2 + (t & 1)];
                const double dx = xs[0 * G + l], wl = xs[1 * G + l], ipy = xs[2 * G + l], py = xs[3 * G + l];
                double* row = PTAB + l * TLD;
                {   // wl dx^n in four interleaved chains
                    const double dx2 = dx * dx, dx4 = dx2 * dx2;
                    double pw[4] = {wl, wl * dx, wl * dx2, wl * dx2 * dx};
#pragma unroll
                    for (int n = 0; n < M2; ++n) {
                        row[n] = pw[n & 3];
                        pw[n & 3] *= dx4;
                    }
                }
                if constexpr (!kLogMain) nell -= fast_log(py);
                wave_sync();
                {   // column sums of the contribution table -> posterior moments
                    const int n0 = l, n1 = l + G;
                    const bool has0 = n0 < M2, has1 = n1 < M2;
                    const double* t0 = PTAB + (has0 ? n0 : 0);
                    const double* t1 = PTAB + (has1 ? n1 : 0);
                    double c0[N], c1[N];
#pragma unroll
                    for (int i = 0; i < N; ++i) { c0[i] = t0[i * TLD]; c1[i] = t1[i * TLD]; }
                    __builtin_amdgcn_sched_barrier(0);
                    double s0[3] = {0.0, 0.0, 0.0}, s1[3] = {0.0, 0.0, 0.0};
#pragma unroll
                    for (int i = 0; i < N; ++i) { s0[i % 3] += c0[i]; s1[i % 3] += c1[i]; }
                    double acc0 = (s0[0] + s0[1]) + s0[2], acc1 = (s1[0] + s1[1]) + s1[2];
                    acc0 *= ipy; acc1 *= ipy;
                    if (has0) { pmom[n0] = acc0; bad |= !finite(acc0); }
                    if (has1) { pmom[n1] = acc1; bad |= !finite(acc1); }
                    out0 = acc0; out1 = acc1;
                }
                wave_sync();
                if constexpr (!kLogMain) bad |= (int)!finite(nell);
                if (gany<G>(bad != 0, grp)) { dead = true; first_nan = t; }
                // the poison decision of the next predict half (a dead filter's flag already says everything)
                pivot_prev = quadrature_fast<N, G, false, kSlPivots>(pmom, l, grp, 0.0, 1.0, xd, wd, lamd, false, true, 0.0, PS, 0);
            } else {
                if (!dead) first_nan = t;   // the pivot flag of the step before: this step is NaN throughout
                dead = true;
                pivot_prev = false;
                for (int n = l; n < M2; n += G) pmom[n] = qnan;
                nell = qnan;
                wave_sync();
            }
            flags[t & 1] = (dead ? kPartnerFlagDead : 0) | (pivot_prev ? kPartnerFlagPivot : 0);
            if (st_m0) a.out_mom[o_mom] = out0;
            if (st_m1) a.out_mom[o_mom + G] = out1;
            o_mom += M2;
        }
        if (has) {
            if (a.t_end >= a.T) {
                if (l == 0) {
                    if constexpr (!kLogMain) a.out_nell[b] = nell;
                    if (a.out_first_nan) a.out_first_nan[b] = first_nan;
                }
            } else {
                for (int n = l; n < M2; n += G) a.c_mom[(size_t)b * M2 + n] = pmom[n];
                if (l == 0) {
                    if constexpr (!kLogMain) a.c_nell[b] = nell;
                    a.c_first_nan[b] = first_nan;
                }
            }
        }
    }
}

}  // namespace mfs
