// capi_1d.hip -- the 1-D moment filters of the C ABI (include/mfs_hip.h): the plan and its kernel choice, chunked launches and
// their hipGraph capture, the host-pointer filter, the gradient, the quadrature and the characteristic function; and the
// definitions of the 1-D launcher tables (registry.hpp).  No kernel header is included.
#include <hip/hip_runtime.h>

#include <cstring>

#include "host_run.hpp"

namespace mfs {
KernelEntry g_table[MFS_MAX_N + 1][kSlots];
FastEntry g_fast[MFS_MAX_N + 1][4];
}  // namespace mfs

namespace {

using mfs::fail;

int check_model(const mfs_model_1d* m, int mode) {
    if (!m) return fail(MFS_EINVAL, "model is NULL");
    if (m->trans_kind != MFS_TRANS_OPERATOR && m->trans_kind != MFS_TRANS_GAUSSIAN)
        return fail(MFS_EINVAL, "unknown trans_kind %d", m->trans_kind);
    if (m->umap != MFS_U_IDENTITY && m->umap != MFS_U_TANH) return fail(MFS_EINVAL, "unknown umap %d", m->umap);
    if (m->degree < 0 || m->degree > MFS_MAX_DEGREE)
        return fail(MFS_EUNSUPPORTED, "polynomial degree %d outside [0, %d]", m->degree, MFS_MAX_DEGREE);
    if (m->trans_kind == MFS_TRANS_OPERATOR) {
        if (m->n_terms < 1 || m->n_terms > MFS_MAX_TERMS)
            return fail(MFS_EUNSUPPORTED, "n_terms %d outside [1, %d]", m->n_terms, MFS_MAX_TERMS);
        if (m->n_rows != m->n_terms + 1) return fail(MFS_EINVAL, "operator table needs n_rows = n_terms + 1");
    } else if (m->n_rows != 2) {
        return fail(MFS_EINVAL, "gaussian table needs n_rows = 2");
    }
    if (m->lik_kind < 0 || m->lik_kind > MFS_LIK_GAUSSIAN) return fail(MFS_EINVAL, "unknown lik_kind %d", m->lik_kind);
    if (m->n_lik < 1 || m->n_lik > MFS_MAX_LIK) return fail(MFS_EINVAL, "n_lik %d outside [1, %d]", m->n_lik, MFS_MAX_LIK);
    if (!m->coef || !m->lik) return fail(MFS_EINVAL, "model tables are NULL");
    if ((mode & 0xff) < MFS_MODE_RAW || (mode & 0xff) > MFS_MODE_SCALED || (mode & ~(0xff | MFS_MODE_ODD_TAIL)))
        return fail(MFS_EINVAL, "unknown mode %d", mode);
    return MFS_OK;
}

// Kernel choice.  Default: the register-resident fast path with the smallest lane group that holds the N + 1 rows of
// the extended Hankel matrix; stable = 1 and odd moment counts run its extended variant (the LDL^T completion only changes
// a rule when a pivot is not > 0: that rule alone takes the dense route, inside the same kernel).  MFS_SOLVER=dense uses
// the LDS-tile dense path throughout.  MFS_LANES_PER_FILTER=16|32|64 overrides the group width (experiments; with
// stable = 1 or an odd count a non-default width runs the dense path -- the extended variant exists for the default only).
int pick_slot(int N, int stable, int odd_tail = 0) {
    bool dense = false;
    if (const char* e = getenv("MFS_SOLVER")) dense = dense || (strcmp(e, "dense") == 0);
    int want = 0;
    if (const char* e = getenv("MFS_LANES_PER_FILTER")) want = atoi(e);
    if ((stable != 0 || odd_tail != 0) && want != 0) dense = true;
    if (dense) {
        int gi = (N <= 16) ? 0 : (N <= 32) ? 1 : 2;
        if (want == 64) gi = 2;
        else if (want == 32 && N <= 32) gi = 1;
        else if (want == 16 && N <= 16) gi = 0;
        return gi;
    }
    int gi = mfs::default_group(N);
    if (want == 64) gi = 2;
    else if (want == 32 && N + 1 <= 32) gi = 1;
    else if (want == 16 && N + 1 <= 16) gi = 0;
    else if (want == 8 && N + 1 <= 8) gi = 3;
    return 3 + gi;
}

// the model of a 1-D filter into the kernel arguments; `coef` and `lik` are the device copies of its tables
void set_model_1d(mfs::Filter1dArgs& a, const mfs_model_1d& m, const double* coef, const double* lik) {
    a.trans_kind = m.trans_kind; a.umap = m.umap; a.n_terms = m.n_terms; a.degree = m.degree; a.n_rows = m.n_rows;
    a.coef_batched = m.coef_batched; a.lik_kind = m.lik_kind; a.n_lik = m.n_lik; a.lik_batched = m.lik_batched;
    a.mean_x_coef = m.mean_x_coef; a.coef = coef; a.lik = lik;
}

}  // namespace

struct mfs_plan_1d {
    mfs_model_1d model;  // device pointers inside
    int mode, N, T, B, stable, chunk, device, extra;
    int G, fpb, grid, lds_bytes, lds_doubles;
    // the kernel build the plan runs, resolved once at creation (resolve_launch): its launcher, the launcher's LDS argument
    // (bytes per block for the dense path, doubles per filter for the fast one) and its MFS_BUILD_* code
    mfs::Filter1dLaunch launch = nullptr;
    int launch_lds = 0, build = MFS_BUILD_DENSE, traits = MFS_TRAITS_RUNTIME;
    // partner-wave variant (filter1d_partner.hpp): `launch` and `grid` are the variant's, and the one-wave build it stands in for
    // stays at hand for the runs it does not cover (MFS_PREDICT_RULE=recompute, read at every run)
    int partner = 0, one_wave_grid = 0;
    mfs::Filter1dFastLaunch one_wave_launch = nullptr;
    double* d_coef = nullptr;
    double* d_lik = nullptr;
    double* c_mom = nullptr;
    double* c_mean = nullptr;
    double* c_scale = nullptr;
    double* c_nell = nullptr;
    int32_t* c_first_nan = nullptr;
    double* c_lam = nullptr;
    hipStream_t own_stream = nullptr;   // created on first use (run() without a caller stream, graph capture)
    // cached graph for the last set of run() pointers
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    const void* key[10] = {nullptr};
    int key_m0_batched = -1;
};

extern "C" {

// ---------------------------------------------------------------------------------------------------------------
// plans
// ---------------------------------------------------------------------------------------------------------------
// `quiesced`: the caller has already synchronised every stream the plan's buffers were used on
static void destroy_plan_1d(mfs_plan_1d* p, bool quiesced) {
    hipSetDevice(p->device);
    if (!quiesced) hipDeviceSynchronize();   // what hipFree did implicitly: pool blocks must be idle when they go back
    if (p->exec) hipGraphExecDestroy(p->exec);
    if (p->graph) hipGraphDestroy(p->graph);
    // model tables and carry state come from the device pool (pool.hpp): a plan per call costs no hipMalloc / hipFree
    mfs::BlockPool<false>& pool = mfs::device_state(p->device).device;
    for (void* b : {(void*)p->d_coef, (void*)p->d_lik, (void*)p->c_mom, (void*)p->c_mean, (void*)p->c_scale,
                    (void*)p->c_nell, (void*)p->c_first_nan, (void*)p->c_lam})
        pool.release(b);
    if (p->own_stream) hipStreamDestroy(p->own_stream);
    delete p;
}

int mfs_plan_1d_destroy(mfs_plan_1d* p) {
    if (p) destroy_plan_1d(p, false);
    return MFS_OK;
}

// The one place that picks the kernel build of a 1-D plan.  Dense slot: its LDS-tile kernel.  Fast slot: blocks are single
// waves, so with at most one per SIMD (grid <= 4 x compute units) the wide-register one-wave builds cost nothing -- the
// specialised one (table in registers, straight-line halves: filter1d_fast.hpp) where the plain kernel's table shape has
// one, else the generic one where the order has one; otherwise the two-wave build.  MFS_FAST_BUILD=generic skips the
// specialised builds (A/B switch, like MFS_PREDICT_RULE).  A specialised build exists a second time with the model's step
// switches compiled in (StepTraits) for a few (table shape, mode, u-map, law) combinations: the plan takes it where its model
// is one of them, MFS_FAST_TRAITS=runtime keeps the run-time-traits build.  Where a fixed-traits build has a partner-wave variant
// (N = 14, 15: 512-thread workgroups of four main and four partner waves) the plan takes that, under the same batch condition
// -- one workgroup per compute unit is one main wave per SIMD; MFS_FAST_PARTNER=0 keeps the one-wave build.
static void resolve_launch(mfs_plan_1d* p, int slot, bool ext) {
    if (slot < 3) {
        p->launch = mfs::g_table[p->N][slot].filter; p->launch_lds = p->lds_bytes; p->build = MFS_BUILD_DENSE;
        return;
    }
    const mfs::FastEntry& fe = mfs::g_fast[p->N][slot - 3];
    int cus = 0;   // (hipDeviceGetAttribute: one integer, not the whole property structure, per plan)
    const bool one_wave = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, p->device) == hipSuccess &&
                          p->grid <= 4 * cus;
    mfs::Filter1dFastLaunch spec = nullptr, wide = one_wave ? (ext ? fe.ext_wide : fe.wide) : nullptr;
    if (one_wave && !ext && ((p->model.degree + 4) & ~3) <= mfs::kSpecTop) {
        const int shape = mfs::spec_shape_index((p->model.trans_kind == MFS_TRANS_OPERATOR) ? p->model.n_terms : -1);
        const char* e = getenv("MFS_FAST_BUILD");
        if (shape >= 0 && !(e && strcmp(e, "generic") == 0)) spec = fe.spec[shape];   // null but for the default group of N = 14..16
        const int ti = mfs::traits_index(p->mode, p->model.umap, p->model.lik_kind);
        const char* et = getenv("MFS_FAST_TRAITS");
        if (spec && ti != MFS_TRAITS_RUNTIME && !(et && strcmp(et, "runtime") == 0) && fe.spec_traits[shape][ti - 1]) {
            spec = fe.spec_traits[shape][ti - 1];
            p->traits = ti;
            const char* ep = getenv("MFS_FAST_PARTNER");
            const int lds = mfs::partner_lds_bytes(p->lds_doubles, fe.partner_doubles);
            if (fe.partner[shape][ti - 1] && !(ep && strcmp(ep, "0") == 0) && lds <= mfs::kPartnerLdsMax) {
                p->partner = 1;
                p->one_wave_launch = spec; p->one_wave_grid = p->grid;
                spec = fe.partner[shape][ti - 1];
                p->fpb = mfs::kPartnerFilters;
                p->grid = (p->B + p->fpb - 1) / p->fpb;
                p->lds_bytes = lds;
            }
        }
    }
    p->launch = spec ? spec : wide ? wide : ext ? fe.ext : fe.filter;
    p->launch_lds = p->lds_doubles;
    p->build = spec ? MFS_BUILD_FAST_ONE_WAVE_SPEC : wide ? MFS_BUILD_FAST_ONE_WAVE : MFS_BUILD_FAST;
}

int mfs_plan_1d_create(mfs_plan_1d** plan, const mfs_model_1d* model, int mode, int N, int T, int B, int stable,
                       int chunk, int device) {
    if (!plan) return fail(MFS_EINVAL, "plan is NULL");
    *plan = nullptr;
    if (int rc = check_model(model, mode)) return rc;
    if (N < 2 || N > MFS_MAX_N) return fail(MFS_EUNSUPPORTED, "N = %d outside [2, %d]", N, MFS_MAX_N);
    if (T < 0 || B < 0) return fail(MFS_EINVAL, "negative T or B");
    if (chunk < 0) return fail(MFS_EINVAL, "negative chunk");
    const int extra = (mode & MFS_MODE_ODD_TAIL) ? 1 : 0;
    mode &= 0xff;
    if (extra && chunk != 0 && chunk < T) return fail(MFS_EUNSUPPORTED, "an odd moment count runs in one launch (chunk = 0)");
    const int slot = pick_slot(N, stable, extra);
    const mfs::KernelEntry& ke = mfs::g_table[N][slot];
    if (!ke.quad) return fail(MFS_EUNSUPPORTED, "no kernel compiled for N = %d", N);
    HIP_TRY(hipSetDevice(device));

    mfs_plan_1d* p = new mfs_plan_1d();
    p->model = *model;
    p->mode = mode; p->N = N; p->T = T; p->B = B; p->stable = stable; p->device = device; p->extra = extra;
    p->chunk = (chunk == 0 || chunk > T) ? T : chunk;
    p->G = ke.lanes_per_filter;
    p->fpb = ke.waves_per_block * (64 / p->G);
    p->grid = (B + p->fpb - 1) / p->fpb;
    p->lds_doubles = ke.lds_doubles_per_filter;
    if (slot >= 3) p->lds_doubles += ((model->degree + 4) & ~3) * 10;  // fast path: + model table [ceil4(degree + 1)][kCoefRows]
    const bool ext = slot >= 3 && (stable != 0 || extra != 0);   // fast path, extended variant
    if (ext) {
        if (!mfs::g_fast[N][slot - 3].ext) { delete p; return fail(MFS_EUNSUPPORTED, "no extended kernel for N = %d", N); }
        p->lds_doubles += mfs::g_fast[N][slot - 3].ext_shift;
    }
    p->lds_bytes = p->fpb * p->lds_doubles * 8;
    resolve_launch(p, slot, ext);

    const size_t ncoef = (size_t)(model->coef_batched ? B : 1) * model->n_rows * (model->degree + 1);
    const size_t nlik = (size_t)(model->lik_batched ? B : 1) * model->n_lik;
    hipError_t e = hipSuccess;
    mfs::BlockPool<false>& pool = mfs::device_state(device).device;
    auto alloc = [&](void** d, size_t bytes) { if (e == hipSuccess) e = pool.acquire(d, bytes); };
    alloc((void**)&p->d_coef, ncoef * 8);
    alloc((void**)&p->d_lik, nlik * 8);
    alloc((void**)&p->c_mom, (size_t)B * 2 * N * 8);
    alloc((void**)&p->c_mean, (size_t)B * 8);
    alloc((void**)&p->c_scale, (size_t)B * 8);
    alloc((void**)&p->c_nell, (size_t)B * 8);
    alloc((void**)&p->c_first_nan, (size_t)B * 4);
    if (p->chunk < T && slot >= 3) alloc((void**)&p->c_lam, (size_t)B * 2 * p->G * 8);
    if (e == hipSuccess) e = hipMemcpy(p->d_coef, model->coef, ncoef * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->d_lik, model->lik, nlik * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        destroy_plan_1d(p, true);
        return fail(e == hipErrorOutOfMemory ? MFS_ENOMEM : MFS_EHIP, "plan setup failed: %s", hipGetErrorString(e));
    }
    p->model.coef = p->d_coef;
    p->model.lik = p->d_lik;
    *plan = p;
    return MFS_OK;
}

int mfs_plan_1d_geometry(const mfs_plan_1d* p, int* lanes_per_filter, int* filters_per_block, int* grid,
                         int* lds_bytes_per_block) {
    if (!p) return fail(MFS_EINVAL, "plan is NULL");
    if (lanes_per_filter) *lanes_per_filter = p->G;
    if (filters_per_block) *filters_per_block = p->fpb;
    if (grid) *grid = p->grid;
    if (lds_bytes_per_block) *lds_bytes_per_block = p->lds_bytes;
    return MFS_OK;
}

int mfs_plan_1d_kernel_build(const mfs_plan_1d* p, int* build) {
    if (!p || !build) return fail(MFS_EINVAL, "plan or build is NULL");
    *build = p->build;
    return MFS_OK;
}

int mfs_plan_1d_kernel_partner(const mfs_plan_1d* p, int* partner) {
    if (!p || !partner) return fail(MFS_EINVAL, "plan or partner is NULL");
    *partner = p->partner;
    return MFS_OK;
}

int mfs_plan_1d_kernel_traits(const mfs_plan_1d* p, int* traits) {
    if (!p || !traits) return fail(MFS_EINVAL, "plan or traits is NULL");
    *traits = p->traits;
    return MFS_OK;
}

int mfs_partner_placement(uint64_t* workgroups, uint64_t* mismatches) {
    if (!workgroups || !mismatches) return fail(MFS_EINVAL, "workgroups or mismatches is NULL");
    uint64_t sum[2] = {0, 0};
    for (int N = 0; N <= MFS_MAX_N; ++N)          // every translation unit with partner kernels holds its own counters
        for (int gi = 0; gi < 4; ++gi)
            if (mfs::PartnerPlacementRead read = mfs::g_fast[N][gi].partner_placement) {
                unsigned long long c[2] = {0, 0};
                HIP_TRY(read(c));
                sum[0] += c[0]; sum[1] += c[1];
            }
    *workgroups = sum[0]; *mismatches = sum[1];
    return MFS_OK;
}

// one launch of the plan's kernel build.  The partner-wave variant has no recomputed predict-half rule: such a run takes the
// one-wave build the variant stands in for.
static hipError_t plan_launch(const mfs_plan_1d* p, const mfs::Filter1dArgs& a, hipStream_t s) {
    if (p->partner && a.recompute_rule) return p->one_wave_launch(a, p->one_wave_grid, p->launch_lds, s);
    return p->launch(a, p->grid, p->launch_lds, s);
}

static int enqueue_chunks(mfs_plan_1d* p, const mfs::Filter1dArgs& base, hipStream_t s) {
    mfs::Filter1dArgs a = base;
    int t0 = 0;
    do {  // (an empty measurement sequence still takes its one launch: nell = 0, nothing else to write)
        a.t_begin = t0;
        a.t_end = (t0 + p->chunk < p->T) ? t0 + p->chunk : p->T;
        hipError_t e = plan_launch(p, a, s);
        if (e != hipSuccess) return fail(MFS_EHIP, "kernel launch failed: %s", hipGetErrorString(e));
    } while ((t0 += p->chunk) < p->T);
    return MFS_OK;
}

// the kernel arguments of a run of the plan, but for the step range
static mfs::Filter1dArgs plan_args(const mfs_plan_1d* p, const mfs::FilterRun& run) {
    mfs::Filter1dArgs a;
    memset(&a, 0, sizeof(a));
    a.mode = p->mode; a.T = p->T; a.B = p->B; a.stable = p->stable; a.extra = p->extra;
    set_model_1d(a, p->model, p->model.coef, p->model.lik);
    mfs::set_run(a, p->mode, run);
    a.c_mom = p->c_mom; a.c_mean = p->c_mean; a.c_scale = p->c_scale; a.c_nell = p->c_nell;
    a.c_first_nan = p->c_first_nan;
    a.c_lam = p->c_lam;
    if (const char* e = getenv("MFS_PREDICT_RULE")) a.recompute_rule = (strcmp(e, "recompute") == 0);   // A/B switch
    return a;
}

int mfs_plan_1d_run(mfs_plan_1d* p, const double* d_m0, int m0_batched, const double* d_mean0,
                    const double* d_scale0, const double* d_ys, double* d_out_moments, double* d_out_means,
                    double* d_out_scales, double* d_out_nell, int32_t* d_out_first_nan, void* stream) {
    if (!p) return fail(MFS_EINVAL, "plan is NULL");
    // (checked before the empty batch returns, where the N-D runs check after it: this entry point asks for ys whenever
    //  T > 0, and the code an existing call returns stays)
    if (int rc = mfs::check_run_pointers(p->mode, d_m0, d_mean0, d_scale0, d_ys, d_out_nell, p->T, 1)) return rc;
    if (p->B == 0) return MFS_OK;
    HIP_TRY(hipSetDevice(p->device));
    const int nchunks = (p->T + p->chunk - 1) / (p->chunk > 0 ? p->chunk : 1);
    if (!p->own_stream && (!stream || nchunks > 1)) HIP_TRY(hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking));
    hipStream_t s = stream ? (hipStream_t)stream : p->own_stream;

    const mfs::Filter1dArgs a = plan_args(p, mfs::FilterRun{d_m0, m0_batched, d_mean0, d_scale0, d_ys, d_out_moments, d_out_means,
                                                             d_out_scales, d_out_nell, d_out_first_nan});
    if (nchunks <= 1) return enqueue_chunks(p, a, s);  // one launch: a graph adds only replay overhead

    // several chunk launches: capture them once into a hipGraph keyed on the buffer set, then replay
    const void* key[10] = {d_m0, d_mean0, d_scale0, d_ys, d_out_moments, d_out_means, d_out_scales, d_out_nell,
                           d_out_first_nan, nullptr};
    const bool hit = p->exec && memcmp(key, p->key, sizeof(key)) == 0 && p->key_m0_batched == m0_batched;
    if (!hit) {
        if (p->exec) { hipGraphExecDestroy(p->exec); p->exec = nullptr; }
        if (p->graph) { hipGraphDestroy(p->graph); p->graph = nullptr; }
        HIP_TRY(hipStreamBeginCapture(p->own_stream, hipStreamCaptureModeThreadLocal));
        int rc = enqueue_chunks(p, a, p->own_stream);
        hipError_t e = hipStreamEndCapture(p->own_stream, &p->graph);
        if (rc != MFS_OK) return rc;
        if (e != hipSuccess) return fail(MFS_EHIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
        HIP_TRY(hipGraphInstantiate(&p->exec, p->graph, nullptr, nullptr, 0));
        memcpy(p->key, key, sizeof(key));
        p->key_m0_batched = m0_batched;
    }
    HIP_TRY(hipGraphLaunch(p->exec, s));
    return MFS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// host-pointer convenience path
// ---------------------------------------------------------------------------------------------------------------
// Device staging comes from the library's pool, streams / events from its context cache (mfs::Staging): no hipMalloc,
// hipFree, hipStreamCreate or hipEventCreate on a steady-state call (SURVEY.md section 8b "Ownership").
int mfs_filter_1d(const mfs_model_1d* model, int mode, int N, int T, int B, const double* m0, int m0_batched,
                  const double* mean0, const double* scale0, const double* ys, int stable, double* out_moments,
                  double* out_means, double* out_scales, double* out_nell, int32_t* out_first_nan, int device,
                  void* stream) {
    const int extra = (mode & MFS_MODE_ODD_TAIL) ? 1 : 0, full_mode = mode;
    mode &= 0xff;
    if (int rc = mfs::check_run_pointers(mode, m0, mean0, scale0, ys, out_nell, T, B)) return rc;
    const size_t M2 = 2 * (size_t)N + extra;     // doubles per moment row
    const int nchunks = extra ? 1 : mfs::host_chunks(device, T, B, M2, out_moments != nullptr);
    const int chunk = (nchunks > 1) ? (T + nchunks - 1) / nchunks : 0;
    mfs_plan_1d* p = nullptr;
    if (int rc = mfs_plan_1d_create(&p, model, full_mode, N, T, B, stable, chunk, device)) return rc;
    struct PlanGuard { mfs_plan_1d* p; ~PlanGuard() { destroy_plan_1d(p, true); } } guard{p};  // (every exit below is quiesced)
    if (B == 0) return MFS_OK;

    mfs::Staging st(device, stream, true);
    const mfs::FilterRun run = mfs::stage_filter_run(st, mode, B, T, m0_batched ? B : 1, M2, 1, 1, 0, m0, m0_batched, mean0,
                                                     scale0, ys, out_moments, out_means, out_scales, out_nell, out_first_nan);
    // same chunking, same carry and therefore the same bits as the plan's graph of chunk launches
    mfs::Filter1dArgs a = plan_args(p, run);
    const int rc = mfs::run_streaming_out(st, T, B, nchunks, M2, out_moments, run.out_mom, [&](int t0, int t1) {
        a.t_begin = t0; a.t_end = t1;
        const hipError_t e = plan_launch(p, a, st.s);
        return (e == hipSuccess) ? MFS_OK : fail(MFS_EHIP, "kernel launch failed: %s", hipGetErrorString(e));
    });
    if (rc == MFS_OK) st.download();
    return st.finish("mfs_filter_1d", rc);
}

int mfs_filter_1d_grad(const mfs_model_1d* model, const double* dcoef, const double* dlik, int n_par, int mode, int N,
                       int T, int B, const double* m0, int m0_batched, const double* mean0, const double* scale0,
                       const double* ys, double* out_nell, double* out_grad, int32_t* out_first_nan, int device,
                       void* stream) {
    if (int rc = check_model(model, mode)) return rc;
    if (mode & MFS_MODE_ODD_TAIL) return fail(MFS_EUNSUPPORTED, "the gradient entry point takes 2N moments");
    if (n_par < 1 || n_par > mfs::kGradMaxP) return fail(MFS_EUNSUPPORTED, "n_par = %d outside [1, %d]", n_par, mfs::kGradMaxP);
    if (N < 2 || N > mfs::kGradMaxN)
        return fail(MFS_EUNSUPPORTED, "N = %d outside [2, %d] for the gradient kernel", N, mfs::kGradMaxN);
    if (T < 0 || B < 0) return fail(MFS_EINVAL, "negative T or B");
    if (!dcoef || !dlik || !out_grad) return fail(MFS_EINVAL, "NULL buffer");
    if (int rc = mfs::check_run_pointers(mode, m0, mean0, scale0, ys, out_nell, T, B)) return rc;
    if (B == 0) return MFS_OK;
    mfs::Filter1dGradLaunch launch = mfs::g_grad_table[N][n_par];
    if (!launch) return fail(MFS_EUNSUPPORTED, "no gradient kernel compiled for N = %d, n_par = %d", N, n_par);
    HIP_TRY(hipSetDevice(device));
    mfs::Staging st(device, stream, true);
    const size_t ncoef = (size_t)model->n_rows * (model->degree + 1), nlik = (size_t)model->n_lik;
    const size_t nbc = model->coef_batched ? B : 1, nbl = model->lik_batched ? B : 1;
    mfs::Filter1dGradArgs ga;
    memset(&ga, 0, sizeof(ga));
    mfs::Filter1dArgs& a = ga.f;
    a.mode = mode; a.T = T; a.B = B; a.t_begin = 0; a.t_end = T;
    set_model_1d(a, *model, st.in(model->coef, nbc * ncoef * 8), st.in(model->lik, nbl * nlik * 8));
    ga.n_par = n_par; ga.dcoef = st.in(dcoef, nbc * n_par * ncoef * 8); ga.dlik = st.in(dlik, nbl * n_par * nlik * 8);
    // the plain filter's run with no moments, means or scales to write
    mfs::set_run(a, mode, mfs::stage_filter_run(st, mode, B, T, m0_batched ? B : 1, 2 * (size_t)N, 1, 1, 0, m0, m0_batched, mean0,
                                                scale0, ys, nullptr, nullptr, nullptr, out_nell, out_first_nan));
    ga.out_grad = st.out(out_grad, (size_t)B * n_par * 8);
    if (st.err == hipSuccess) st.err = launch(ga, B, st.s);      // (the launcher knows its lanes per filter)
    st.download();
    return st.finish("mfs_filter_1d_grad", MFS_OK);
}

int mfs_quadrature_1d(int N, int B, const double* ms, const double* mean, const double* scale, int stable,
                      double* out_weights, double* out_nodes, int device, void* stream) {
    if (N < 2 || N > MFS_MAX_N) return fail(MFS_EUNSUPPORTED, "N = %d outside [2, %d]", N, MFS_MAX_N);
    if (B < 0) return fail(MFS_EINVAL, "negative B");
    if (B == 0) return MFS_OK;
    if (!ms || !out_weights || !out_nodes) return fail(MFS_EINVAL, "NULL buffer");
    const int slot = pick_slot(N, stable);
    const mfs::KernelEntry& ke = mfs::g_table[N][slot];
    if (!ke.quad) return fail(MFS_EUNSUPPORTED, "no kernel compiled for N = %d", N);
    HIP_TRY(hipSetDevice(device));
    const int G = ke.lanes_per_filter;
    const int fpb = ke.waves_per_block * (64 / G);
    // the completed rule of stable = 1 needs the extended tile
    const mfs::FastEntry* ext = (slot >= 3 && stable != 0) ? &mfs::g_fast[N][slot - 3] : nullptr;
    if (ext && !ext->quad_ext) return fail(MFS_EUNSUPPORTED, "no extended quadrature kernel for N = %d", N);
    const int quad_lds = fpb * (ext ? ext->quad_ext_lds : slot >= 3 ? 2 * N : ke.lds_doubles_per_filter) * 8;
    mfs::Staging st(device, stream, false);   // on the caller's stream, null included
    const size_t B8 = (size_t)B * 8;     // (mean and scale: no block where the caller has none)
    const mfs::Quad1dArgs a{B, stable, st.in(ms, 2 * N * B8), mean ? st.in(mean, B8) : nullptr, scale ? st.in(scale, B8) : nullptr,
                            st.out(out_weights, N * B8), st.out(out_nodes, N * B8)};
    if (st.err == hipSuccess) st.err = (ext ? ext->quad_ext : ke.quad)(a, (B + fpb - 1) / fpb, quad_lds, st.s);
    st.download();
    return st.finish("mfs_quadrature_1d", MFS_OK);
}

// ---------------------------------------------------------------------------------------------------------------
// characteristic function from moments, host pointers
// ---------------------------------------------------------------------------------------------------------------
int mfs_characteristic_1d(int N, int count, const double* ms, const double* mean, const double* scale, int nz,
                          const double* zs, double* out, int device, void* stream) {
    if (N < 2 || N > MFS_MAX_N) return fail(MFS_EUNSUPPORTED, "N = %d outside [2, %d]", N, MFS_MAX_N);
    if (count < 0 || nz < 0) return fail(MFS_EINVAL, "negative count or nz");
    if (count == 0 || nz == 0) return MFS_OK;
    if (!ms || !zs || !out) return fail(MFS_EINVAL, "NULL buffer");
    const int gi = mfs::default_group(N);
    mfs::Cf1dLaunch launch = mfs::g_fast[N][gi].cf;
    if (!launch) return fail(MFS_EUNSUPPORTED, "no kernel compiled for N = %d", N);
    HIP_TRY(hipSetDevice(device));
    const int fpb = 64 / mfs::group_lanes(gi);
    mfs::Staging st(device, stream, false);   // on the caller's stream, null included
    const size_t c8 = (size_t)count * 8;     // (mean and scale: no block where the caller has none)
    const mfs::Cf1dArgs a{count, nz, st.in(ms, 2 * N * c8), mean ? st.in(mean, c8) : nullptr, scale ? st.in(scale, c8) : nullptr,
                          st.in(zs, (size_t)nz * 8), st.out(out, 2 * nz * c8)};
    if (st.err == hipSuccess) st.err = launch(a, (count + fpb - 1) / fpb, fpb * 2 * N * 8, st.s);
    st.download();
    return st.finish("mfs_characteristic_1d", MFS_OK);
}

}  // extern "C"
