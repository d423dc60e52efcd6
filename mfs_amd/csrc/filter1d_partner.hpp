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
// Every floating-point operation that feeds an output is the one-wave build's, in its order: the blocks of the two halves
// are the functions filter1d_fast_kernel calls for a fixed-traits build (filter1d_fast.hpp, above the kernel), split between
// the roles -- only the staging of the model tables is a copy -- and quadrature_fast is called as it is
// there (the partner's call keeps only the pivots, as the predict half of the one-wave builds does); the SL bits this variant
// adds to its calls (kSlFreezeX, kSlPivMin) drop selects and compares whose results nothing reads, no arithmetic.
// First step of a run (no atoms): the main wave runs the cold full rule on the moments it loads, as the one-wave builds do.
// Start of a chunk: the partner eliminates the carried moments before the first barrier (the flag of step t_begin).
// MFS_PREDICT_RULE=recompute keeps the one-wave launcher (capi.hip).
#pragma once
#include "filter1d_fast.hpp"

namespace mfs {

// Decided by leave-one-out builds (compile-time switches MFS_PARTNER_AB_* that existed up to commit ac4d42d; the series of
// DESIGN.md section 6 were taken with them): log p_y and nell on the partner, the partner's flags consumed inside the next
// step, an eigenvalue loop that freezes only x of a converged lane (kSlFreezeX), the poison flag from a running minimum of
// the pivots (kSlPivMin).  (No s_setprio for the main waves: it measured slower.)

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
        if (has) {   // stage the model tables (twin: filter1d_fast_kernel)
            const int J1 = a.degree + 1;
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
        double mean = 0.0, scale = 1.0;
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
                first_nan = a.c_first_nan[b];
                if (a.c_lam) {
                    gA = a.c_lam[((size_t)b * 2 + 0) * G + l];
                    gW = a.c_lam[((size_t)b * 2 + 1) * G + l];
                    have_atoms = true;
                }
            }
        }
        wave_sync();
        double tabr[kSpecTop][SpecRows<SPEC>::SR];
        LikRegs lpr;
        // (an absent filter reads whatever its tile holds: nothing of it is ever stored)
        load_table_regs<SPEC>(coef, tabr);
        load_lik_regs(lp, lpr);
        const bool st_mean = has && a.out_mean && (l == 0);
        size_t o_mean = (size_t)b * a.T + a.t_begin;
        const double* yrow = a.ys + (size_t)b * a.T;
        bool dead = !has || (first_nan >= 0);
        asm volatile("" : "+v"(mean), "+v"(scale), "+v"(gA), "+v"(gW), "+v"(first_nan));   // the carry waits, in front of the loop
        double ywin = 0.0;
        constexpr int kSlUpdate = kSlEigLoop | kSlFreezeX | kSlPivMin;
        constexpr int trans_kind = (SPEC > 0) ? MFS_TRANS_OPERATOR : MFS_TRANS_GAUSSIAN;
        // the late flag: the flag word read behind barrier t and the mean of step t, both settled inside step t + 1
        int fl_prev = 0;
        double mean_prev = 0.0;
        const auto settle = [&]() __attribute__((always_inline)) {
            if (dead || fl_prev != 0) {
                dead = true;
                mean = qnan; scale = qnan; mean_prev = qnan;
            }
            if (st_mean) a.out_mean[o_mean] = mean_prev;
            o_mean += 1;
        };

        for (int t = a.t_begin; t < a.t_end; ++t) {
            const double y = y_window<G>(yrow, has, l, t, a.t_begin, a.t_end, ywin);
            double* xs = xch + (t & 1) * 4 * G;
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
                    table_rows<SPEC>(tabr, u, rows);
                    double mu, var;
                    transition_mu_var(trans_kind, a.mean_x_coef, x, rows, mu, var);
                    mean = gsum<G>(w * mu);
                    c = mean;
                    double* row = TAB + l * TLD;
                    if (trans_kind == MFS_TRANS_OPERATOR) {
                        operator_moments<(SPEC > 0) ? SPEC : 2, M2>(rows, x - c, w, inv_sc, node, row);
                    } else {
                        normal_closure_row<M2>(w, mu, var, c, inv_sc, row);
                    }
                    wave_sync();
                    double pm0, pm1;   // (the predicted moments are no output)
                    column_sums<N, G, M2, TLD, false>(TAB, mom, l, 0, 1.0, 0, bad, pm0, pm1);
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
            if (t > a.t_begin) settle();
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
                    const double dx = posterior_atoms<N, G>(x, c, inv_sc, wl, ipy, node, gA, gW);
                    have_atoms = true;
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
            // write the word again, and waited for and acted on inside step t + 1, or behind the loop
            fl_prev = flags[(t + 1) & 1];
            mean_prev = mean;
        }
        if (a.t_end > a.t_begin) settle();   // the last step's mean, before the carry is written
        if (has) {
            if (a.t_end < a.T) {
                if (a.c_lam) { a.c_lam[((size_t)b * 2 + 0) * G + l] = gA; a.c_lam[((size_t)b * 2 + 1) * G + l] = gW; }
                if (l == 0) { a.c_mean[b] = mean; a.c_scale[b] = scale; }
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
            nell = a.c_nell[b];
            first_nan = a.c_first_nan[b];
        }
        wave_sync();
        bool dead = !has || (first_nan >= 0);
        if (!dead && a.t_begin != 0)   // the flag of step t_begin: the elimination the one-wave builds run in its predict half
            pivot_prev = quadrature_fast<N, G, false, kSlPivMin>(pmom, l, grp, 0.0, 1.0, xd, wd, lamd, false, true, 0.0, PS, 0);
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
                power_row<M2, false>(wl, dx, PTAB + l * TLD);
                nell -= fast_log(py);
                wave_sync();
                column_sums<N, G, M2, TLD, false>(PTAB, pmom, l, 1, ipy, 0, bad, out0, out1);   // posterior moments
                wave_sync();
                bad |= (int)!finite(nell);
                if (gany<G>(bad != 0, grp)) { dead = true; first_nan = t; }
                // the poison decision of the next predict half (a dead filter's flag already says everything)
                pivot_prev = quadrature_fast<N, G, false, kSlPivMin>(pmom, l, grp, 0.0, 1.0, xd, wd, lamd, false, true, 0.0, PS, 0);
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
                    a.out_nell[b] = nell;
                    if (a.out_first_nan) a.out_first_nan[b] = first_nan;
                }
            } else {
                for (int n = l; n < M2; n += G) a.c_mom[(size_t)b * M2 + n] = pmom[n];
                if (l == 0) {
                    a.c_nell[b] = nell;
                    a.c_first_nan[b] = first_nan;
                }
            }
        }
    }
}

}  // namespace mfs
