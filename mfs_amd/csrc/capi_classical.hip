// capi_classical.hip -- the classical baselines of the C ABI (include/mfs_hip.h), host pointers: the bootstrap particle filters
// (d = 1, 2) and the Gaussian filters (sigma-point and EKF; d = 1, 2), which share the checks on a Gaussian-transition model
// (kernels: particle_kernel.hpp, particle_nd_kernel.hpp, gaussfilter_kernel.hpp, reached through registry.hpp only).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <utility>

#include "host_run.hpp"

using mfs::fail;

// ---------------------------------------------------------------------------------------------------------------
// bootstrap particle filters.  The two entries share their argument check, their work buffers and the step driver below;
// each stages its own model and summaries
// ---------------------------------------------------------------------------------------------------------------
extern "C" int mfs_pf_draws(uint64_t seed, int t, int tag, int draw, int count, double* out_uniform, double* out_normal,
                            int device) {
    if (count < 0 || t < 0 || tag < 0 || draw < 0) return fail(MFS_EINVAL, "mfs_pf_draws: negative count, t, tag or draw");
    if (count == 0) return MFS_OK;
    if (!out_uniform || !out_normal) return fail(MFS_EINVAL, "mfs_pf_draws: NULL buffer");
    HIP_TRY(hipSetDevice(device));
    mfs::Staging st(device, nullptr, true);
    double *d_u = st.out(out_uniform, (size_t)count * 8), *d_z = st.out(out_normal, (size_t)count * 8);
    if (st.err == hipSuccess) st.err = mfs::launch_pf_draws(seed, t, tag, draw, count, d_u, d_z, st.s);
    st.download();
    return st.finish("mfs_pf_draws", MFS_OK);
}

static thread_local double g_pf_split_ms[5];   // propagate, offsets, resample, cf, finalize of this thread's last call

extern "C" int mfs_pf_last_split_ms(double* out) {
    if (!out) return fail(MFS_EINVAL, "mfs_pf_last_split_ms: NULL buffer");
    for (int k = 0; k < 5; ++k) out[k] = g_pf_split_ms[k];
    return MFS_OK;
}

// ---- what the particle filters of every state dimension share on the host
// the arguments both entries take; `mix_spread` is the mixture's third array (mix_var, mix_chol), named in the message
static int check_pf_args(const char* me, int n, int T, int B, int resampling, int n_mix, const double* mix_cumw,
                         const double* mix_mean, const double* mix_spread, const char* spread_name, const double* init_samples) {
    if (n < 1 || T < 1 || B < 1) return fail(MFS_EINVAL, "%s: n = %d, T = %d, B = %d (all >= 1)", me, n, T, B);
    if (n > MFS_PF_MAX_PARTICLES) return fail(MFS_EUNSUPPORTED, "%s: n = %d particles > %d", me, n, MFS_PF_MAX_PARTICLES);
    if (resampling != MFS_RESAMPLE_STRATIFIED && resampling != MFS_RESAMPLE_SYSTEMATIC)
        return fail(MFS_EINVAL, "%s: unknown resampling code %d", me, resampling);
    if (n_mix < 0 || n_mix > MFS_PF_MAX_MIX) return fail(MFS_EINVAL, "%s: n_mix = %d outside [0, %d]", me, n_mix, MFS_PF_MAX_MIX);
    if (n_mix == 0 && !init_samples) return fail(MFS_EINVAL, "%s: n_mix = 0 needs init_samples", me);
    if (n_mix > 0 && (!mix_cumw || !mix_mean || !mix_spread))
        return fail(MFS_EINVAL, "%s: mix_cumw / mix_mean / %s must not be NULL", me, spread_name);
    return MFS_OK;
}

// What does not depend on the state dimension, into the arguments of either filter (Args: PfArgs / PfNdArgs) and of the
// `offsets` kernel, which is returned: the call's shape, the seeds (uploaded), the weight scan, the block totals, their
// offsets, the weight sums, and nell (zeroed) and first_nan (-1), which the call gives back
template <typename Args>
static mfs::PfOffsetsArgs pf_work_buffers(mfs::Staging& st, Args& a, int n, int T, int nB, int resampling, const uint64_t* seeds,
                                          double* out_nell, int32_t* out_first_nan) {
    const size_t B = (size_t)nB;
    mfs::PfOffsetsArgs o;
    memset(&o, 0, sizeof(o));
    a.n = o.n = n; a.T = T; a.B = o.B = nB; a.nblk = o.nblk = mfs::pf_blocks(n); a.nseg = mfs::pf_segments(n);
    a.resampling = resampling;
    a.seeds = st.in(seeds, B * 8); a.wscan = st.work(B * n * 8);
    a.wpart = o.wpart = st.work(B * o.nblk * 8); a.woffs = o.woffs = st.work(B * o.nblk * 8); a.wtot = o.wtot = st.work(B * 8);
    o.nell = st.out(out_nell, B * 8); o.first_nan = st.out(out_first_nan, B * 4, 0, mfs::Staging::kAlways);
    if (st.err == hipSuccess) st.err = hipMemsetAsync(o.nell, 0, B * 8, st.s);
    if (st.err == hipSuccess) st.err = hipMemsetAsync(o.first_nan, 0xff, B * 4, st.s);   // -1
    return o;
}

// the initial law into the arguments of either filter: the mixture's three arrays (`dim` doubles per mean, dim x dim per
// spread) side by side in one block, or the caller's samples; a.mix_cumw, a.mix_mean and `a_spread` point into the block
template <typename Args>
static void pf_initial_law(mfs::Staging& st, Args& a, const double*& a_spread, size_t dim, const double* mix_cumw,
                           const double* mix_mean, const double* mix_spread, const double* init_samples, size_t nb_init) {
    const size_t k = (size_t)a.n_mix;
    if (k == 0) { a.init = st.in(init_samples, nb_init * a.n * dim * 8); return; }
    double* d_mix = st.work((1 + dim + dim * dim) * k * 8);
    st.h2d(d_mix, mix_cumw, k * 8); st.h2d(d_mix + k, mix_mean, k * dim * 8); st.h2d(d_mix + (1 + dim) * k, mix_spread, k * dim * dim * 8);
    a.mix_cumw = d_mix; a.mix_mean = d_mix + k; a_spread = d_mix + (1 + dim) * k;
}

// The T steps of a call on st.s: begin(t), then the step's five launches launch(0) .. launch(4) (propagate, offsets, resample,
// the summary pass, finalize), then end().  MFS_PF_SPLIT=1 (the benchmark tools; read at every call): an event after every
// launch and a wait per step, so that mfs_pf_last_split_ms can report the time of each of the five kernels; the results are
// the same bits, the call is slower by the waits
template <typename Begin, typename Launch, typename End>
static void pf_run_steps(mfs::Staging& st, int T, Begin&& begin, Launch&& launch, End&& end) {
    const char* split_env = getenv("MFS_PF_SPLIT");
    const bool split = split_env && split_env[0] == '1';
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < 6 && split && st.err == hipSuccess; ++k) st.err = hipEventCreate(&ev[k]);
    for (int k = 0; k < 5; ++k) g_pf_split_ms[k] = 0.0;
    auto mark = [&](int k) { if (split && st.err == hipSuccess) st.err = hipEventRecord(ev[k], st.s); };
    for (int t = 0; t < T && st.err == hipSuccess; ++t) {
        begin(t);
        mark(0);
        for (int k = 0; k < 5; ++k) {
            if (st.err == hipSuccess) st.err = launch(k);
            mark(k + 1);
        }
        if (split && st.err == hipSuccess) st.err = hipEventSynchronize(ev[5]);
        for (int k = 0; k < 5 && split && st.err == hipSuccess; ++k) {
            float ms = 0.f;
            st.err = hipEventElapsedTime(&ms, ev[k], ev[k + 1]);
            g_pf_split_ms[k] += (double)ms;
        }
        end();
    }
    for (int k = 0; k < 6; ++k)
        if (ev[k]) (void)hipEventDestroy(ev[k]);
}

// ---- Gaussian-transition models, as the baselines take them (the particle filters here, the Gaussian filters below).  `me`
// is the entry's name and `what` the thing that needs the model ("proposal", "filter")
static int check_gaussian_model_1d(const char* me, const char* what, const mfs_model_1d* model) {
    if (!model) return fail(MFS_EINVAL, "%s: NULL model", me);
    if (model->trans_kind != MFS_TRANS_GAUSSIAN || model->n_rows != 2)
        return fail(MFS_EINVAL, "%s: the %s needs a MFS_TRANS_GAUSSIAN model (trans_kind %d, n_rows %d)", me, what,
                    model->trans_kind, model->n_rows);
    if (model->degree < 0 || model->degree > MFS_MAX_DEGREE) return fail(MFS_EINVAL, "%s: degree %d outside [0, %d]", me, model->degree, MFS_MAX_DEGREE);
    if (model->umap != MFS_U_IDENTITY && model->umap != MFS_U_TANH) return fail(MFS_EINVAL, "%s: unknown umap %d", me, model->umap);
    if (model->lik_kind < MFS_LIK_BERNOULLI_LOGISTIC || model->lik_kind > MFS_LIK_GAUSSIAN)
        return fail(MFS_EINVAL, "%s: lik_kind %d is not a 1-D likelihood", me, model->lik_kind);
    if (model->n_lik < 1 || model->n_lik > MFS_MAX_LIK) return fail(MFS_EINVAL, "%s: n_lik %d outside [1, %d]", me, model->n_lik, MFS_MAX_LIK);
    return MFS_OK;
}

// such a model into the kernel arguments (Args: PfArgs / GfArgs, which name these fields alike), but for its tables
template <typename Args>
static void set_gaussian_model_1d(Args& a, const mfs_model_1d& m) {
    a.umap = m.umap; a.degree = m.degree; a.coef_batched = m.coef_batched != 0; a.lik_kind = m.lik_kind;
    a.n_lik = m.n_lik; a.lik_batched = m.lik_batched != 0; a.mean_x_coef = m.mean_x_coef;
}

// d = 2: the model and its table, then its likelihood factors 0 .. n_factors - 1.  An entry's own restrictions on the factors
// (how many, which columns; MFS_EUNSUPPORTED where the model is valid but not run) come between the two
static int check_gaussian_model_nd(const char* me, const char* what, const mfs_model_nd* model) {
    if (!model) return fail(MFS_EINVAL, "%s: NULL model", me);
    if (model->d != 2) return fail(MFS_EUNSUPPORTED, "%s: d = %d (the filter runs d = 2; d = 1 goes through %.*s1d)", me, model->d,
                                       (int)strlen(me) - 2, me);
    if (model->trans_kind != MFS_ND_TRANS_GAUSSIAN)
        return fail(MFS_EINVAL, "%s: the %s needs a MFS_ND_TRANS_GAUSSIAN model (trans_kind %d)", me, what, model->trans_kind);
    if (model->extent < 1 || model->extent > MFS_ND_MAX_EXTENT_HI)
        return fail(MFS_EINVAL, "%s: extent %d outside [1, %d]", me, model->extent, MFS_ND_MAX_EXTENT_HI);
    return MFS_OK;
}

static int check_gaussian_factors_nd(const char* me, const mfs_model_nd* model, int n_factors) {
    for (int f = 0; f < n_factors; ++f) {
        if (model->fac_kind[f] < MFS_LIK_BERNOULLI_LOGISTIC || model->fac_kind[f] > MFS_LIK_GAUSSIAN)
            return fail(MFS_EINVAL, "%s: factor %d: kind %d is not a likelihood of one state component", me, f, model->fac_kind[f]);
        if (model->fac_component[f] < 0 || model->fac_component[f] > 1)
            return fail(MFS_EINVAL, "%s: factor %d: fac_component %d outside [0, 1]", me, f, model->fac_component[f]);
    }
    return MFS_OK;
}

extern "C" int mfs_particle_filter_1d(const mfs_model_1d* model, int n, int T, int B, int resampling, const uint64_t* seeds,
                                      int n_mix, const double* mix_cumw, const double* mix_mean, const double* mix_var,
                                      const double* init_samples, int init_batched, const double* ys, int nz, const double* zs,
                                      double* out_samples, double* out_means, double* out_vars, double* out_cfs,
                                      double* out_nell, int32_t* out_first_nan, int device, void* stream) {
    const char* me = "mfs_particle_filter_1d";
    if (const int rc = check_pf_args(me, n, T, B, resampling, n_mix, mix_cumw, mix_mean, mix_var, "mix_var", init_samples)) return rc;
    if (const int rc = check_gaussian_model_1d(me, "proposal", model)) return rc;
    for (int k = 0; k < n_mix; ++k)
        if (!std::isfinite(mix_var[k]) || !(mix_var[k] > 0.0) || !std::isfinite(mix_mean[k]))
            return fail(MFS_EINVAL, "%s: mixture component %d is not finite with variance > 0", me, k);
    if (nz < 0 || (nz > 0 && (!zs || !out_cfs))) return fail(MFS_EINVAL, "%s: nz = %d needs zs and out_cfs", me, nz);
    if (!model->coef || !model->lik || !seeds || !ys || !out_means || !out_vars || !out_nell)
        return fail(MFS_EINVAL, "%s: model tables / seeds / ys / out_means / out_vars / out_nell must not be NULL", me);
    HIP_TRY(hipSetDevice(device));

    // a uniformly spaced frequency grid lets the cf kernel rotate between true sincos evaluations
    int z_uniform = 0;
    double dz = 0.0;
    if (nz > 1) {
        dz = (zs[nz - 1] - zs[0]) / (double)(nz - 1);
        double zmax = 0.0, dev = 0.0;
        for (int k = 0; k < nz; ++k) {
            zmax = std::fmax(zmax, std::fabs(zs[k]));
            dev = std::fmax(dev, std::fabs(zs[k] - (zs[0] + (double)k * dz)));
        }
        z_uniform = std::isfinite(dz) && dev <= 8.0 * 2.220446049250313e-16 * zmax;
    }

    const size_t bn = (size_t)B * n, bt = (size_t)B * T, J1 = (size_t)model->degree + 1;
    const size_t nb_coef = model->coef_batched ? (size_t)B : 1, nb_lik = model->lik_batched ? (size_t)B : 1;
    mfs::Staging st(device, stream, true);
    mfs::PfArgs a;
    memset(&a, 0, sizeof(a));
    set_gaussian_model_1d(a, *model);
    a.coef = st.in(model->coef, nb_coef * 2 * J1 * 8); a.lik = st.in(model->lik, nb_lik * model->n_lik * 8);
    a.ys = st.in(ys, bt * 8);
    mfs::PfOffsetsArgs o = pf_work_buffers(st, a, n, T, B, resampling, seeds, out_nell, out_first_nan);
    a.n_mix = n_mix; a.init_batched = init_batched != 0;
    pf_initial_law(st, a, a.mix_var, 1, mix_cumw, mix_mean, mix_var, init_samples, init_batched ? (size_t)B : 1);
    a.nz = nz; a.z_uniform = z_uniform; a.dz = dz;
    if (nz > 0) a.zs = st.in(zs, (size_t)nz * 8);
    a.x = st.work(bn * 8); a.x2 = st.work(bn * 8);
    a.xpart = st.work((size_t)B * a.nblk * 8); a.vpart = st.work((size_t)B * a.nseg * 8);
    if (nz > 0) a.cfpart = st.work((size_t)B * a.nseg * nz * 16);
    a.out_samples = st.out(out_samples, bt * n * 8);
    a.out_means = st.out(out_means, bt * 8); a.out_vars = st.out(out_vars, bt * 8);
    if (nz > 0) a.out_cfs = st.out(out_cfs, bt * nz * 16);
    if (st.err == hipSuccess) st.err = mfs::launch_pf_init(a, st.s);
    pf_run_steps(st, T, [&](int t) { a.t = o.t = t; },
                 [&](int k) {
                     return k == 0 ? mfs::launch_pf_propagate(a, st.s) : k == 1 ? mfs::launch_pf_offsets(o, st.s)
                          : k == 2 ? mfs::launch_pf_resample(a, st.s) : k == 3 ? mfs::launch_pf_cf(a, st.s)
                                                                               : mfs::launch_pf_finalize(a, st.s);
                 },
                 [&] { std::swap(a.x, a.x2); });   // the resampled particles are the next step's
    st.download();
    return st.finish(me, MFS_OK);
}

// the same for a two-dimensional state (kernels: particle_nd_kernel.hpp)
extern "C" int mfs_particle_filter_nd(const mfs_model_nd* model, int n, int T, int B, int resampling, const uint64_t* seeds,
                                      int n_mix, const double* mix_cumw, const double* mix_mean, const double* mix_chol,
                                      const double* init_samples, int init_batched, const double* ys, double* out_samples,
                                      double* out_means, double* out_covs, double* out_nell, int32_t* out_first_nan,
                                      int device, void* stream) {
    const char* me = "mfs_particle_filter_nd";
    if (const int rc = check_pf_args(me, n, T, B, resampling, n_mix, mix_cumw, mix_mean, mix_chol, "mix_chol", init_samples)) return rc;
    if (const int rc = check_gaussian_model_nd(me, "proposal", model)) return rc;
    if (model->n_factors < 1 || model->n_factors > MFS_ND_MAX_FACTORS)
        return fail(MFS_EINVAL, "%s: n_factors %d outside [1, %d]", me, model->n_factors, MFS_ND_MAX_FACTORS);
    if (model->ny < 1 || model->ny > 2) return fail(MFS_EINVAL, "%s: ny %d outside [1, 2]", me, model->ny);
    if (const int rc = check_gaussian_factors_nd(me, model, model->n_factors)) return rc;
    for (int f = 0; f < model->n_factors; ++f)
        if (model->fac_ycol[f] < 0 || model->fac_ycol[f] >= model->ny)
            return fail(MFS_EINVAL, "%s: factor %d: fac_ycol %d outside [0, ny = %d)", me, f, model->fac_ycol[f], model->ny);
    for (int k = 0; k < n_mix; ++k) {
        const double* L = mix_chol + 4 * k;
        if (!std::isfinite(L[0]) || !(L[0] > 0.0) || !std::isfinite(L[3]) || !(L[3] > 0.0) || !std::isfinite(L[2]) ||
            !std::isfinite(mix_mean[2 * k]) || !std::isfinite(mix_mean[2 * k + 1]))
            return fail(MFS_EINVAL, "%s: mixture component %d is not finite with a factor of diagonal > 0", me, k);
    }
    if (!model->coef || !model->lik || !seeds || !ys || !out_means || !out_covs || !out_nell)
        return fail(MFS_EINVAL, "%s: model tables / seeds / ys / out_means / out_covs / out_nell must not be NULL", me);
    HIP_TRY(hipSetDevice(device));

    const int ny = model->ny, nf = model->n_factors;
    const size_t table = (size_t)MFS_ND_TABLE_ROWS(model->n_terms) * model->extent * model->extent;
    const size_t bn = (size_t)B * n, bt = (size_t)B * T;
    const size_t nb_coef = model->coef_batched ? (size_t)B : 1, nb_lik = model->lik_batched ? (size_t)B : 1;
    mfs::Staging st(device, stream, true);
    mfs::PfNdArgs a;
    memset(&a, 0, sizeof(a));
    a.extent = model->extent; a.coef_stride = (int)table; a.coef_batched = model->coef_batched != 0;
    a.n_factors = nf; a.ny = ny; a.lik_batched = model->lik_batched != 0;
    for (int f = 0; f < nf; ++f) {
        a.fac_kind[f] = model->fac_kind[f]; a.fac_component[f] = model->fac_component[f]; a.fac_ycol[f] = model->fac_ycol[f];
    }
    a.coef = st.in(model->coef, nb_coef * table * 8); a.lik = st.in(model->lik, nb_lik * nf * MFS_MAX_LIK * 8);
    a.ys = st.in(ys, bt * ny * 8);
    mfs::PfOffsetsArgs o = pf_work_buffers(st, a, n, T, B, resampling, seeds, out_nell, out_first_nan);
    a.n_mix = n_mix; a.init_batched = init_batched != 0;
    pf_initial_law(st, a, a.mix_chol, 2, mix_cumw, mix_mean, mix_chol, init_samples, init_batched ? (size_t)B : 1);
    a.x = st.work(bn * 16); a.x2 = st.work(bn * 16);
    a.xpart = st.work((size_t)B * a.nblk * 16); a.cpart = st.work((size_t)B * a.nseg * 24);
    a.out_samples = st.out(out_samples, bt * n * 16);
    a.out_means = st.out(out_means, bt * 16); a.out_covs = st.out(out_covs, bt * 32);
    if (st.err == hipSuccess) st.err = mfs::launch_pfnd_init(a, st.s);
    pf_run_steps(st, T, [&](int t) { a.t = o.t = t; },
                 [&](int k) {
                     return k == 0 ? mfs::launch_pfnd_propagate(a, st.s) : k == 1 ? mfs::launch_pf_offsets(o, st.s)
                          : k == 2 ? mfs::launch_pfnd_resample(a, st.s) : k == 3 ? mfs::launch_pfnd_cov(a, st.s)
                                                                                 : mfs::launch_pfnd_finalize(a, st.s);
                 },
                 [&] { std::swap(a.x, a.x2); });   // the resampled particles are the next step's
    st.download();
    return st.finish(me, MFS_OK);
}

// ---------------------------------------------------------------------------------------------------------------
// Gaussian filters: sigma-point filter and EKF
// ---------------------------------------------------------------------------------------------------------------
// what the two entry points share once `a` describes the model: the rule, the staging, the launch and the copies back
static int run_gauss_filter(const char* me, mfs::GfArgs& a, const double* coef, size_t coef_doubles, const double* lik,
                            size_t lik_doubles, const double* xi, const double* w, const double* m0, const double* P0,
                            const double* ys, double* out_means, double* out_covs, double* out_nells, int32_t* out_first_nan,
                            int device, void* stream) {
    const int d = a.d, T = a.T, B = a.B;
    if (a.method != MFS_GF_SIGMA_POINT && a.method != MFS_GF_EKF) return fail(MFS_EINVAL, "%s: unknown method %d", me, a.method);
    if (T < 1 || B < 1) return fail(MFS_EINVAL, "%s: T = %d, B = %d (both >= 1)", me, T, B);
    if (a.method == MFS_GF_SIGMA_POINT) {
        if (a.n_points < 1 || a.n_points > MFS_GF_MAX_POINTS)
            return fail(MFS_EUNSUPPORTED, "%s: n_points = %d outside [1, %d]", me, a.n_points, MFS_GF_MAX_POINTS);
        if (!xi || !w) return fail(MFS_EINVAL, "%s: the sigma-point method needs xi and w", me);
        a.lanes = mfs::gf_lanes(a.n_points);
    } else {
        a.n_points = 0;
        a.lanes = 1;
    }
    if (!coef || !lik || !m0 || !P0 || !ys || !out_nells)
        return fail(MFS_EINVAL, "%s: model tables / m0 / v0 / ys / out_nells must not be NULL", me);
    HIP_TRY(hipSetDevice(device));
    const size_t bt = (size_t)B * T, nb_init = a.init_batched ? (size_t)B : 1, np = (size_t)a.n_points;
    mfs::Staging st(device, stream, true);
    a.coef = st.in(coef, coef_doubles * 8); a.lik = st.in(lik, lik_doubles * 8);
    if (np) { a.xi = st.in(xi, np * d * 8); a.w = st.in(w, np * 8); }
    a.m0 = st.in(m0, nb_init * d * 8); a.P0 = st.in(P0, nb_init * d * d * 8); a.ys = st.in(ys, bt * 8);
    a.out_means = st.out(out_means, bt * d * 8); a.out_covs = st.out(out_covs, bt * d * d * 8);
    a.out_nells = st.out(out_nells, bt * 8); a.out_first_nan = st.out(out_first_nan, (size_t)B * 4);
    if (st.err == hipSuccess) st.err = mfs::launch_gauss_filter(a, st.s);
    st.download();
    return st.finish(me, MFS_OK);
}

extern "C" int mfs_gaussian_filter_1d(const mfs_model_1d* model, int method, int n_points, const double* xi, const double* w,
                                      int T, int B, const double* m0, const double* v0, int init_batched, const double* ys,
                                      double* out_means, double* out_vars, double* out_nells, int32_t* out_first_nan,
                                      int device, void* stream) {
    const char* me = "mfs_gaussian_filter_1d";
    if (const int rc = check_gaussian_model_1d(me, "filter", model)) return rc;
    mfs::GfArgs a;
    memset(&a, 0, sizeof(a));
    a.d = 1; a.method = method; a.n_points = n_points; a.T = T; a.B = B; a.init_batched = init_batched != 0;
    set_gaussian_model_1d(a, *model);
    const size_t nb = (B > 0) ? (size_t)B : 0;
    return run_gauss_filter(me, a, model->coef, (a.coef_batched ? nb : 1) * 2 * (model->degree + 1), model->lik,
                            (a.lik_batched ? nb : 1) * model->n_lik, xi, w, m0, v0, ys, out_means, out_vars, out_nells,
                            out_first_nan, device, stream);
}

extern "C" int mfs_gaussian_filter_nd(const mfs_model_nd* model, int method, int n_points, const double* xi, const double* w,
                                      int T, int B, const double* m0, const double* P0, int init_batched, const double* ys,
                                      double* out_means, double* out_covs, double* out_nells, int32_t* out_first_nan,
                                      int device, void* stream) {
    const char* me = "mfs_gaussian_filter_nd";
    if (const int rc = check_gaussian_model_nd(me, "filter", model)) return rc;
    if (model->n_factors != 1 || model->ny != 1 || model->fac_ycol[0] != 0)
        return fail(MFS_EUNSUPPORTED, "%s: one likelihood factor of a scalar measurement is supported (n_factors %d, ny %d)", me,
                    model->n_factors, model->ny);
    if (model->fac_kind[0] == MFS_LIK_BEARING_GAUSSIAN || model->fac_component[0] == 2)
        return fail(MFS_EUNSUPPORTED, "%s: a likelihood factor of both state components is not supported", me);
    if (const int rc = check_gaussian_factors_nd(me, model, 1)) return rc;
    if (model->coef_batched) return fail(MFS_EUNSUPPORTED, "%s: per-replicate transition tables (coef_batched) are not supported at d = 2", me);
    mfs::GfArgs a;
    memset(&a, 0, sizeof(a));
    a.d = 2; a.method = method; a.n_points = n_points; a.T = T; a.B = B; a.init_batched = init_batched != 0;
    a.extent = model->extent; a.component = model->fac_component[0]; a.lik_kind = model->fac_kind[0]; a.n_lik = MFS_MAX_LIK;
    a.lik_batched = model->lik_batched != 0;
    const size_t nb = (B > 0) ? (size_t)B : 0;
    // blocks 0..4 of the table (mu_0, mu_1, S_00, S_01, S_11) are all the filter reads
    return run_gauss_filter(me, a, model->coef, (size_t)5 * model->extent * model->extent, model->lik,
                            (a.lik_batched ? nb : 1) * MFS_MAX_LIK, xi, w, m0, P0, ys, out_means, out_covs, out_nells,
                            out_first_nan, device, stream);
}
