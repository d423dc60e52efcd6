// capi.hip -- the C ABI of libmfs_hip.so (include/mfs_hip.h): argument checking, device staging, chunked launches,
// hipGraph capture.  No compute lives here and no kernel header is included: launchers and argument structs come from registry.hpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <mutex>
#include <string>
#include <vector>

#include "registry.hpp"
#include "staging.hpp"

namespace mfs {
KernelEntry g_table[MFS_MAX_N + 1][kSlots];
FastEntry g_fast[MFS_MAX_N + 1][4];

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
}  // namespace mfs

namespace {

using mfs::fail;

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(MFS_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

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

// what every run needs of its data pointers, device or host (ys only where there is a measurement to read)
int check_run_pointers(int mode, const double* m0, const double* mean0, const double* scale0, const double* ys,
                       const double* out_nell, int T, int B) {
    if (!m0 || !out_nell || (T > 0 && B > 0 && !ys)) return fail(MFS_EINVAL, "m0 / ys / out_nell must not be NULL");
    if (mode != MFS_MODE_RAW && !mean0) return fail(MFS_EINVAL, "mean0 is required in central and scaled modes");
    if (mode == MFS_MODE_SCALED && !scale0) return fail(MFS_EINVAL, "scale0 is required in scaled mode");
    return MFS_OK;
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

int mfs_version(void) { return MFS_ABI_VERSION; }
const char* mfs_last_error(void) { return mfs::g_err.c_str(); }

int mfs_device_count(int* count) {
    if (!count) return fail(MFS_EINVAL, "count is NULL");
    HIP_TRY(hipGetDeviceCount(count));
    return MFS_OK;
}
int mfs_set_device(int device) { HIP_TRY(hipSetDevice(device)); return MFS_OK; }
int mfs_device_synchronize(void) { HIP_TRY(hipDeviceSynchronize()); return MFS_OK; }
int mfs_device_name(int device, char* buf, int buflen) {
    if (!buf || buflen <= 0) return fail(MFS_EINVAL, "bad buffer");
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, device));
    snprintf(buf, buflen, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount);
    return MFS_OK;
}
int mfs_malloc(void** dptr, uint64_t bytes) {
    if (!dptr) return fail(MFS_EINVAL, "dptr is NULL");
    hipError_t e = hipMalloc(dptr, bytes ? bytes : 8);
    if (e != hipSuccess) return fail(MFS_ENOMEM, "hipMalloc(%llu) failed: %s", (unsigned long long)bytes, hipGetErrorString(e));
    return MFS_OK;
}
int mfs_free(void* dptr) { if (dptr) HIP_TRY(hipFree(dptr)); return MFS_OK; }
int mfs_memcpy_h2d(void* dst, const void* src, uint64_t bytes, void* stream) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return MFS_OK;
}
int mfs_memcpy_d2h(void* dst, const void* src, uint64_t bytes, void* stream) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return MFS_OK;
}
int mfs_memset(void* dst, int value, uint64_t bytes, void* stream) {
    HIP_TRY(hipMemsetAsync(dst, value, bytes, (hipStream_t)stream));
    return MFS_OK;
}
int mfs_stream_create(void** stream) {
    if (!stream) return fail(MFS_EINVAL, "stream is NULL");
    HIP_TRY(hipStreamCreateWithFlags((hipStream_t*)stream, hipStreamNonBlocking));
    return MFS_OK;
}
int mfs_stream_destroy(void* stream) { if (stream) HIP_TRY(hipStreamDestroy((hipStream_t)stream)); return MFS_OK; }
int mfs_stream_synchronize(void* stream) { HIP_TRY(hipStreamSynchronize((hipStream_t)stream)); return MFS_OK; }
int mfs_event_create(void** event) {
    if (!event) return fail(MFS_EINVAL, "event is NULL");
    HIP_TRY(hipEventCreate((hipEvent_t*)event));
    return MFS_OK;
}
int mfs_event_destroy(void* event) { if (event) HIP_TRY(hipEventDestroy((hipEvent_t)event)); return MFS_OK; }
int mfs_event_record(void* event, void* stream) { HIP_TRY(hipEventRecord((hipEvent_t)event, (hipStream_t)stream)); return MFS_OK; }
int mfs_event_elapsed_ms(void* start, void* stop, float* ms) {
    if (!ms) return fail(MFS_EINVAL, "ms is NULL");
    HIP_TRY(hipEventSynchronize((hipEvent_t)stop));
    HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return MFS_OK;
}

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

int mfs_plan_1d_kernel_traits(const mfs_plan_1d* p, int* traits) {
    if (!p || !traits) return fail(MFS_EINVAL, "plan or traits is NULL");
    *traits = p->traits;
    return MFS_OK;
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

static mfs::Filter1dArgs plan_args(const mfs_plan_1d* p, const double* d_m0, int m0_batched, const double* d_mean0,
                                    const double* d_scale0, const double* d_ys, double* d_out_moments,
                                    double* d_out_means, double* d_out_scales, double* d_out_nell,
                                    int32_t* d_out_first_nan) {
    mfs::Filter1dArgs a;
    memset(&a, 0, sizeof(a));
    a.mode = p->mode; a.T = p->T; a.B = p->B; a.stable = p->stable; a.extra = p->extra;
    a.trans_kind = p->model.trans_kind; a.umap = p->model.umap; a.n_terms = p->model.n_terms;
    a.degree = p->model.degree; a.n_rows = p->model.n_rows; a.coef_batched = p->model.coef_batched;
    a.lik_kind = p->model.lik_kind; a.n_lik = p->model.n_lik; a.lik_batched = p->model.lik_batched;
    a.mean_x_coef = p->model.mean_x_coef; a.coef = p->model.coef; a.lik = p->model.lik;
    a.m0 = d_m0; a.m0_batched = m0_batched; a.mean0 = d_mean0; a.scale0 = d_scale0; a.ys = d_ys;
    a.c_mom = p->c_mom; a.c_mean = p->c_mean; a.c_scale = p->c_scale; a.c_nell = p->c_nell;
    a.c_first_nan = p->c_first_nan;
    a.c_lam = p->c_lam;
    if (const char* e = getenv("MFS_PREDICT_RULE")) a.recompute_rule = (strcmp(e, "recompute") == 0);   // A/B switch
    a.out_mom = d_out_moments; a.out_mean = (p->mode != MFS_MODE_RAW) ? d_out_means : nullptr;
    a.out_scale = (p->mode == MFS_MODE_SCALED) ? d_out_scales : nullptr;
    a.out_nell = d_out_nell; a.out_first_nan = d_out_first_nan;
    return a;
}

int mfs_plan_1d_run(mfs_plan_1d* p, const double* d_m0, int m0_batched, const double* d_mean0,
                    const double* d_scale0, const double* d_ys, double* d_out_moments, double* d_out_means,
                    double* d_out_scales, double* d_out_nell, int32_t* d_out_first_nan, void* stream) {
    if (!p) return fail(MFS_EINVAL, "plan is NULL");
    // (checked before the empty batch returns: this entry point asks for ys whenever T > 0)
    if (int rc = check_run_pointers(p->mode, d_m0, d_mean0, d_scale0, d_ys, d_out_nell, p->T, 1)) return rc;
    if (p->B == 0) return MFS_OK;
    HIP_TRY(hipSetDevice(p->device));
    const int nchunks = (p->T + p->chunk - 1) / (p->chunk > 0 ? p->chunk : 1);
    if (!p->own_stream && (!stream || nchunks > 1)) HIP_TRY(hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking));
    hipStream_t s = stream ? (hipStream_t)stream : p->own_stream;

    const mfs::Filter1dArgs a = plan_args(p, d_m0, m0_batched, d_mean0, d_scale0, d_ys, d_out_moments, d_out_means,
                                          d_out_scales, d_out_nell, d_out_first_nan);
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
// hipMemcpy2DAsync takes a pitch: a row of T x (moments per step) x 8 bytes beyond the runtime's limit (runs of ~1e6 steps and
// more) would fail the whole call, so such runs go out in one linear copy instead (no copy / compute overlap)
static bool pitch_ok(size_t pitch_bytes, int device) {
    int maxp = 0;
    if (hipDeviceGetAttribute(&maxp, hipDeviceAttributeMaxPitch, device) != hipSuccess || maxp <= 0) return pitch_bytes < ((size_t)1 << 31);
    return pitch_bytes <= (size_t)maxp;
}

// How many T-chunks a host entry splits a run into when the moments ([B][T][width] doubles) are streamed out
// (mfs::run_streaming_out): one per 32 MB of them, at most 16.  MFS_HOST_CHUNKS overrides (1 = one launch, copies afterwards).
static int host_chunks(int device, int T, int B, size_t width, bool out_moments) {
    if (B <= 0 || T <= 0 || !pitch_ok((size_t)T * width * 8, device)) return 1;
    int n = out_moments ? (int)((size_t)B * T * width * 8 / ((size_t)32 << 20)) : 0;
    if (const char* e = getenv("MFS_HOST_CHUNKS")) n = atoi(e);
    if (n > 16) n = 16;
    if (n > T) n = T;
    return n < 1 ? 1 : n;
}

// Device staging comes from the library's pool, streams / events from its context cache (mfs::Staging): no hipMalloc,
// hipFree, hipStreamCreate or hipEventCreate on a steady-state call (SURVEY.md section 8b "Ownership").
int mfs_filter_1d(const mfs_model_1d* model, int mode, int N, int T, int B, const double* m0, int m0_batched,
                  const double* mean0, const double* scale0, const double* ys, int stable, double* out_moments,
                  double* out_means, double* out_scales, double* out_nell, int32_t* out_first_nan, int device,
                  void* stream) {
    const int extra = (mode & MFS_MODE_ODD_TAIL) ? 1 : 0, full_mode = mode;
    mode &= 0xff;
    if (int rc = check_run_pointers(mode, m0, mean0, scale0, ys, out_nell, T, B)) return rc;
    const size_t M2 = 2 * (size_t)N + extra, nb = m0_batched ? B : 1;     // doubles per moment row
    const int nchunks = extra ? 1 : host_chunks(device, T, B, M2, out_moments != nullptr);
    const int chunk = (nchunks > 1) ? (T + nchunks - 1) / nchunks : 0;
    mfs_plan_1d* p = nullptr;
    if (int rc = mfs_plan_1d_create(&p, model, full_mode, N, T, B, stable, chunk, device)) return rc;
    struct PlanGuard { mfs_plan_1d* p; ~PlanGuard() { destroy_plan_1d(p, true); } } guard{p};  // (every exit below is quiesced)
    if (B == 0) return MFS_OK;

    mfs::Staging st(device, stream, true);
    double *d_m0 = nullptr, *d_mean0 = nullptr, *d_scale0 = nullptr, *d_ys = nullptr, *d_mom = nullptr,
           *d_means = nullptr, *d_scales = nullptr, *d_nell = nullptr;
    int32_t* d_fn = nullptr;
    st.alloc(&d_m0, nb * M2 * 8);
    st.alloc(&d_mean0, nb * 8);
    st.alloc(&d_scale0, nb * 8);
    st.alloc(&d_ys, (size_t)B * T * 8);
    if (out_moments) st.alloc(&d_mom, (size_t)B * T * M2 * 8);
    if (out_means && mode != MFS_MODE_RAW) st.alloc(&d_means, (size_t)B * T * 8);
    if (out_scales && mode == MFS_MODE_SCALED) st.alloc(&d_scales, (size_t)B * T * 8);
    st.alloc(&d_nell, (size_t)B * 8);
    st.alloc(&d_fn, (size_t)B * 4);
    st.h2d(d_m0, m0, nb * M2 * 8);
    if (mean0) st.h2d(d_mean0, mean0, nb * 8);
    if (scale0) st.h2d(d_scale0, scale0, nb * 8);
    st.h2d(d_ys, ys, (size_t)B * T * 8);

    // same chunking, same carry and therefore the same bits as the plan's graph of chunk launches
    mfs::Filter1dArgs a = plan_args(p, d_m0, m0_batched, d_mean0, d_scale0, d_ys, d_mom, d_means, d_scales, d_nell, d_fn);
    const int rc = mfs::run_streaming_out(st, T, B, nchunks, M2, out_moments, d_mom, [&](int t0, int t1) {
        a.t_begin = t0; a.t_end = t1;
        const hipError_t e = plan_launch(p, a, st.s);
        return (e == hipSuccess) ? MFS_OK : fail(MFS_EHIP, "kernel launch failed: %s", hipGetErrorString(e));
    });
    if (rc == MFS_OK) {
        st.d2h(out_means, d_means, (size_t)B * T * 8);
        st.d2h(out_scales, d_scales, (size_t)B * T * 8);
        st.d2h(out_nell, d_nell, (size_t)B * 8);
        st.d2h(out_first_nan, d_fn, (size_t)B * 4);
    }
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
    if (int rc = check_run_pointers(mode, m0, mean0, scale0, ys, out_nell, T, B)) return rc;
    if (B == 0) return MFS_OK;
    mfs::Filter1dGradLaunch launch = mfs::g_grad_table[N][n_par];
    if (!launch) return fail(MFS_EUNSUPPORTED, "no gradient kernel compiled for N = %d, n_par = %d", N, n_par);
    HIP_TRY(hipSetDevice(device));
    mfs::Staging st(device, stream, true);
    const size_t J1 = (size_t)model->degree + 1, ncoef = (size_t)model->n_rows * J1;
    const size_t nbc = model->coef_batched ? B : 1, nbl = model->lik_batched ? B : 1, nb = m0_batched ? B : 1, M2 = 2 * (size_t)N;
    double *d_coef = nullptr, *d_dcoef = nullptr, *d_lik = nullptr, *d_dlik = nullptr, *d_m0 = nullptr, *d_mean0 = nullptr,
           *d_scale0 = nullptr, *d_ys = nullptr, *d_nell = nullptr, *d_grad = nullptr;
    int32_t* d_fn = nullptr;
    st.alloc(&d_coef, nbc * ncoef * 8); st.alloc(&d_dcoef, nbc * n_par * ncoef * 8);
    st.alloc(&d_lik, nbl * model->n_lik * 8); st.alloc(&d_dlik, nbl * n_par * model->n_lik * 8);
    st.alloc(&d_m0, nb * M2 * 8); st.alloc(&d_mean0, nb * 8); st.alloc(&d_scale0, nb * 8);
    st.alloc(&d_ys, (size_t)B * T * 8); st.alloc(&d_nell, (size_t)B * 8); st.alloc(&d_grad, (size_t)B * n_par * 8);
    st.alloc(&d_fn, (size_t)B * 4);
    st.h2d(d_coef, model->coef, nbc * ncoef * 8); st.h2d(d_dcoef, dcoef, nbc * n_par * ncoef * 8);
    st.h2d(d_lik, model->lik, nbl * model->n_lik * 8); st.h2d(d_dlik, dlik, nbl * n_par * model->n_lik * 8);
    st.h2d(d_m0, m0, nb * M2 * 8);
    if (mean0) st.h2d(d_mean0, mean0, nb * 8);
    if (scale0) st.h2d(d_scale0, scale0, nb * 8);
    st.h2d(d_ys, ys, (size_t)B * T * 8);
    if (st.err == hipSuccess) {
        mfs::Filter1dGradArgs ga;
        memset(&ga, 0, sizeof(ga));
        mfs::Filter1dArgs& a = ga.f;
        a.mode = mode; a.T = T; a.B = B; a.t_begin = 0; a.t_end = T;
        a.trans_kind = model->trans_kind; a.umap = model->umap; a.n_terms = model->n_terms; a.degree = model->degree;
        a.n_rows = model->n_rows; a.coef_batched = model->coef_batched; a.lik_kind = model->lik_kind; a.n_lik = model->n_lik;
        a.lik_batched = model->lik_batched; a.mean_x_coef = model->mean_x_coef; a.coef = d_coef; a.lik = d_lik;
        a.m0 = d_m0; a.m0_batched = m0_batched; a.mean0 = d_mean0; a.scale0 = d_scale0; a.ys = d_ys;
        a.out_nell = d_nell; a.out_first_nan = d_fn;
        ga.n_par = n_par; ga.dcoef = d_dcoef; ga.dlik = d_dlik; ga.out_grad = d_grad;
        st.err = launch(ga, B, st.s);      // (the launcher knows its lanes per filter)
    }
    st.d2h(out_nell, d_nell, (size_t)B * 8); st.d2h(out_grad, d_grad, (size_t)B * n_par * 8); st.d2h(out_first_nan, d_fn, (size_t)B * 4);
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
    double *d_ms = nullptr, *d_mean = nullptr, *d_scale = nullptr, *d_w = nullptr, *d_x = nullptr;
    mfs::Staging st(device, stream, false);   // on the caller's stream, null included
    st.alloc(&d_ms, (size_t)B * 2 * N * 8);
    st.alloc(&d_w, (size_t)B * N * 8);
    st.alloc(&d_x, (size_t)B * N * 8);
    if (mean) st.alloc(&d_mean, (size_t)B * 8);
    if (scale) st.alloc(&d_scale, (size_t)B * 8);
    st.h2d(d_ms, ms, (size_t)B * 2 * N * 8);
    if (mean) st.h2d(d_mean, mean, (size_t)B * 8);
    if (scale) st.h2d(d_scale, scale, (size_t)B * 8);
    if (st.err == hipSuccess) {
        mfs::Quad1dArgs a{B, stable, d_ms, d_mean, d_scale, d_w, d_x};
        st.err = (ext ? ext->quad_ext : ke.quad)(a, (B + fpb - 1) / fpb, quad_lds, st.s);
    }
    st.d2h(out_weights, d_w, (size_t)B * N * 8);
    st.d2h(out_nodes, d_x, (size_t)B * N * 8);
    return st.finish("mfs_quadrature_1d", MFS_OK);
}

// ---------------------------------------------------------------------------------------------------------------
// the staging pool (pool.hpp), as far as callers see it
// ---------------------------------------------------------------------------------------------------------------
int mfs_host_alloc(void** ptr, uint64_t bytes, int device) {
    if (!ptr) return fail(MFS_EINVAL, "ptr is NULL");
    *ptr = nullptr;
    if (device < 0 || device >= mfs::kMaxDevices) return fail(MFS_EINVAL, "device %d outside [0, %d)", device, mfs::kMaxDevices);
    HIP_TRY(hipSetDevice(device));
    hipError_t e = mfs::device_state(device).pinned.acquire(ptr, (size_t)bytes);
    if (e != hipSuccess) return fail(MFS_ENOMEM, "hipHostMalloc(%llu) failed: %s", (unsigned long long)bytes, hipGetErrorString(e));
    return MFS_OK;
}

int mfs_host_free(void* ptr) {
    if (!ptr) return MFS_OK;
    for (int d = 0; d < mfs::kMaxDevices; ++d)
        if (mfs::device_state(d).pinned.release(ptr)) return MFS_OK;
    return fail(MFS_EINVAL, "pointer was not handed out by mfs_host_alloc");
}

int mfs_pool_trim(int device) {
    if (device < 0 || device >= mfs::kMaxDevices) return fail(MFS_EINVAL, "device %d outside [0, %d)", device, mfs::kMaxDevices);
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipDeviceSynchronize());
    mfs::DeviceState& st = mfs::device_state(device);
    st.device.trim();
    st.pinned.trim();
    st.contexts.trim();
    return MFS_OK;
}

int mfs_pool_stats(int device, uint64_t* device_bytes, uint64_t* pinned_bytes, uint64_t* device_allocs, uint64_t* pinned_allocs) {
    if (device < 0 || device >= mfs::kMaxDevices) return fail(MFS_EINVAL, "device %d outside [0, %d)", device, mfs::kMaxDevices);
    mfs::DeviceState& st = mfs::device_state(device);
    const mfs::PoolCounters dc = st.device.counters(), pc = st.pinned.counters();
    if (device_bytes) *device_bytes = dc.cached_bytes;
    if (pinned_bytes) *pinned_bytes = pc.cached_bytes;
    if (device_allocs) *device_allocs = dc.fresh_allocs;
    if (pinned_allocs) *pinned_allocs = pc.fresh_allocs;
    return MFS_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------
// RCCL all-gather of the per-replicate NLL vector.  librccl is dlopen'ed on first use so
// that single-GPU users never pay for loading it.
// ---------------------------------------------------------------------------------------------------------------
namespace {
struct Rccl {
    void* handle = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, mfs_rccl_id, int) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;
std::mutex g_rccl_mu;

int load_rccl() {
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (g_rccl.handle) return MFS_OK;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    for (const char* n : names) { h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
    if (!h) return fail(MFS_ERCCL, "cannot dlopen librccl: %s", dlerror());
    g_rccl.GetUniqueId = (int (*)(void*))dlsym(h, "ncclGetUniqueId");
    g_rccl.CommInitRank = (int (*)(void**, int, mfs_rccl_id, int))dlsym(h, "ncclCommInitRank");
    g_rccl.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(h, "ncclAllGather");
    g_rccl.CommDestroy = (int (*)(void*))dlsym(h, "ncclCommDestroy");
    g_rccl.GetErrorString = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllGather || !g_rccl.CommDestroy)
        return fail(MFS_ERCCL, "librccl lacks an expected symbol");
    g_rccl.handle = h;
    return MFS_OK;
}
#define RCCL_TRY(expr)                                                                                     \
    do {                                                                                                   \
        int r_ = (expr);                                                                                   \
        if (r_ != 0) return fail(MFS_ERCCL, "%s failed: %s", #expr,                                        \
                                 g_rccl.GetErrorString ? g_rccl.GetErrorString(r_) : "rccl error");        \
    } while (0)
}  // namespace

extern "C" {

int mfs_comm_unique_id(mfs_rccl_id* id) {
    if (!id) return fail(MFS_EINVAL, "id is NULL");
    if (int rc = load_rccl()) return rc;
    RCCL_TRY(g_rccl.GetUniqueId(id));
    return MFS_OK;
}

int mfs_comm_init(void** comm, const mfs_rccl_id* id, int nranks, int rank, int device) {
    if (!comm || !id) return fail(MFS_EINVAL, "NULL argument");
    if (rank < 0 || rank >= nranks) return fail(MFS_EINVAL, "rank %d outside [0, %d)", rank, nranks);
    if (int rc = load_rccl()) return rc;
    HIP_TRY(hipSetDevice(device));
    RCCL_TRY(g_rccl.CommInitRank(comm, nranks, *id, rank));
    return MFS_OK;
}

int mfs_allgather_nell(void* comm, const double* d_send, double* d_recv, uint64_t count, void* stream) {
    if (!comm || !d_send || !d_recv) return fail(MFS_EINVAL, "NULL argument");
    if (int rc = load_rccl()) return rc;
    RCCL_TRY(g_rccl.AllGather(d_send, d_recv, (size_t)count, 8 /* ncclFloat64 */, comm, (hipStream_t)stream));
    return MFS_OK;
}

int mfs_comm_destroy(void* comm) {
    if (!comm) return MFS_OK;
    if (int rc = load_rccl()) return rc;
    RCCL_TRY(g_rccl.CommDestroy(comm));
    return MFS_OK;
}

int mfs_memcpy_d2d(void* dst, const void* src, uint64_t bytes, void* stream) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MFS_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------
// N-D filter (d = 2)
// ---------------------------------------------------------------------------------------------------------------
// what the d = 2 and d = 3 plans share: the run's shape and the device copies of the model tables
struct NdPlanBase {
    int mode, N, T, B, device;
    double* d_coef = nullptr;
    double* d_lik = nullptr;
    int32_t* d_inds = nullptr;
};

struct mfs_plan_nd : NdPlanBase {
    mfs::FilterNdLaunch launch = nullptr;   // the kernel family of the model, resolved at creation
    mfs::FilterNdArgs args;   // model part filled at create (device pointers), data pointers per run
};

// pool blocks for the coefficient, likelihood-parameter and Gram / Hankel index tables, and their upload
static hipError_t upload_nd_tables(NdPlanBase* p, const double* coef, size_t ncoef, const double* lik, size_t nlik,
                                   const int32_t* inds, size_t ninds) {
    mfs::BlockPool<false>& pool = mfs::device_state(p->device).device;
    hipError_t e = pool.acquire((void**)&p->d_coef, ncoef * 8);
    if (e == hipSuccess) e = pool.acquire((void**)&p->d_lik, nlik * 8);
    if (e == hipSuccess) e = pool.acquire((void**)&p->d_inds, ninds * 4);
    if (e == hipSuccess && ncoef) e = hipMemcpy(p->d_coef, coef, ncoef * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess && nlik) e = hipMemcpy(p->d_lik, lik, nlik * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->d_inds, inds, ninds * 4, hipMemcpyHostToDevice);
    return e;
}

// the part of the kernel arguments that both model structs describe alike (Args: FilterNdArgs / FilterNd3Args)
template <typename Args, typename Model>
static void fill_nd_args(Args& a, const NdPlanBase* p, const Model* model) {
    memset(&a, 0, sizeof(a));
    a.mode = p->mode; a.T = p->T; a.B = p->B;
    a.D = model->extent; a.n_factors = model->n_factors; a.ny = model->ny;
    for (int f = 0; f < model->n_factors; ++f) {
        a.fac_kind[f] = model->fac_kind[f]; a.fac_comp[f] = model->fac_component[f]; a.fac_ycol[f] = model->fac_ycol[f];
    }
    a.coef_batched = model->coef_batched; a.lik_batched = model->lik_batched;
    a.coef = p->d_coef; a.lik = p->d_lik; a.inds = p->d_inds;
}

static mfs::BlockPool<false>& release_nd_tables(NdPlanBase* p, bool quiesced) {
    hipSetDevice(p->device);
    if (!quiesced) hipDeviceSynchronize();   // pool blocks must be idle when they go back (what hipFree did implicitly)
    mfs::BlockPool<false>& pool = mfs::device_state(p->device).device;
    pool.release(p->d_coef); pool.release(p->d_lik); pool.release(p->d_inds);
    return pool;
}

static void destroy_plan_nd(mfs_plan_nd* p, bool quiesced) {
    release_nd_tables(p, quiesced);
    delete p;
}

extern "C" int mfs_plan_nd_create(mfs_plan_nd** plan, const mfs_model_nd* model, int mode, int N, int T, int B, int z,
                                  const int32_t* multi_indices, const int32_t* inds, int stable, int device) {
    if (!plan) return fail(MFS_EINVAL, "plan is NULL");
    *plan = nullptr;
    if (!model) return fail(MFS_EINVAL, "model is NULL");
    if (model->d != 2) return fail(MFS_EUNSUPPORTED, "the device N-D path supports d = 2 (got %d)", model->d);
    if (mode != MFS_MODE_RAW && mode != MFS_MODE_CENTRAL && mode != MFS_MODE_SCALED)
        return fail(MFS_EINVAL, "unknown moment mode %d", mode);
    if (N < 2 || N > mfs::kNdMaxN) return fail(MFS_EUNSUPPORTED, "N = %d outside [2, %d] for d = 2", N, mfs::kNdMaxN);
    const mfs::NdEntry& ke = mfs::g_nd_table[N];
    if (!ke.launch) return fail(MFS_EUNSUPPORTED, "no N-D kernel compiled for N = %d", N);
    if (model->trans_kind != MFS_ND_TRANS_OPERATOR && model->trans_kind != MFS_ND_TRANS_GAUSSIAN)
        return fail(MFS_EINVAL, "unknown N-D transition kind %d", model->trans_kind);
    if (model->trans_kind == MFS_ND_TRANS_GAUSSIAN && model->n_terms != 5)
        return fail(MFS_EINVAL, "the Gaussian N-D transition carries 5 polynomials (mu_0, mu_1, S_00, S_01, S_11)");
    if (model->n_terms < 0 || model->n_terms > MFS_ND_TERMS_MAX) return fail(MFS_EINVAL, "bad n_terms %d", model->n_terms);
    const int n_rows = MFS_ND_TABLE_ROWS(model->n_terms);     // 16, or 29 when terms with |kappa| > 4 are present (TME order 3)
    if (z != ke.Z) return fail(MFS_EINVAL, "The size of multi_indices %d must match that of the moments %d.", z, ke.Z);
    const int max_extent = (model->trans_kind == MFS_ND_TRANS_OPERATOR && model->n_terms > MFS_ND_TERMS) ? MFS_ND_MAX_EXTENT_HI : MFS_ND_MAX_EXTENT;
    if (model->extent < 1 || model->extent > max_extent)
        return fail(MFS_EUNSUPPORTED, "coefficient extent %d outside [1, %d]", model->extent, max_extent);
    if (model->n_factors < 1 || model->n_factors > MFS_ND_MAX_FACTORS)
        return fail(MFS_EINVAL, "n_factors %d outside [1, %d]", model->n_factors, MFS_ND_MAX_FACTORS);
    if (model->ny < 1 || model->ny > 2) return fail(MFS_EINVAL, "ny %d outside [1, 2]", model->ny);
    for (int f = 0; f < model->n_factors; ++f) {
        const bool joint = model->fac_kind[f] == MFS_LIK_BEARING_GAUSSIAN;     // a factor of both components: component 2
        if (model->fac_kind[f] < 0 || model->fac_kind[f] > MFS_LIK_BEARING_GAUSSIAN || model->fac_n_par[f] < 1 ||
            model->fac_n_par[f] > MFS_MAX_LIK || model->fac_component[f] < 0 || model->fac_component[f] > 2 ||
            (model->fac_component[f] == 2) != joint || model->fac_ycol[f] < 0 || model->fac_ycol[f] >= model->ny)
            return fail(MFS_EINVAL, "bad description of likelihood factor %d", f);
        if (joint && (model->n_factors != 1 || (model->trans_kind == MFS_ND_TRANS_OPERATOR && (model->n_terms > MFS_ND_TERMS || N > 6))))
            return fail(MFS_EUNSUPPORTED, "a likelihood of both state components: one such factor, with a Normal-closure transition or "
                                          "operator tables of TME order <= 2 at N <= 6 (the other kernels' tiles have no room for the "
                                          "node tables)");
    }
    if (T < 0 || B < 0) return fail(MFS_EINVAL, "negative T or B");
    if (!multi_indices || !inds || !model->coef || !model->lik) return fail(MFS_EINVAL, "NULL buffer");
    {   // The kernels compute the gather of quadratures.py:151-152 arithmetically from the graded-lex order of
        // multi_indices.py:139-229 (d = 2: the index of (a0, a1) is (a0 + a1)(a0 + a1 + 1) / 2 + a0); a caller's table must be that one.
        const int S = ke.S;
        auto deg = [](int i) { int m = 0; while ((m + 1) * (m + 2) / 2 <= i) ++m; return m; };
        for (int t = 0; t < 3; ++t)
            for (int i = 0; i < S; ++i)
                for (int j = 0; j < S; ++j) {
                    const int mi = deg(i), mj = deg(j), ui = i - mi * (mi + 1) / 2, uj = j - mj * (mj + 1) / 2;
                    const int M = mi + mj + (t > 0), want = M * (M + 1) / 2 + ui + uj + (t == 1);
                    if (inds[(size_t)t * S * S + i * S + j] != want)
                        return fail(MFS_EUNSUPPORTED, "inds[%d][%d][%d] = %d is not the graded-lexicographic Gram / Hankel table (expected %d)",
                                    t, i, j, inds[(size_t)t * S * S + i * S + j], want);
                }
    }
    // the kernel derives a moment's multi-index from its position: insist on the graded-lex table
    for (int s = 0, zi = 0; s < 2 * N; ++s)
        for (int n0 = 0; n0 <= s; ++n0, ++zi)
            if (multi_indices[2 * zi] != n0 || multi_indices[2 * zi + 1] != s - n0)
                return fail(MFS_EINVAL, "multi_indices is not the graded-lexicographic table of order 2N-1");
    HIP_TRY(hipSetDevice(device));
    mfs_plan_nd* p = new (std::nothrow) mfs_plan_nd();
    if (!p) return fail(MFS_ENOMEM, "out of host memory");
    p->mode = mode; p->N = N; p->T = T; p->B = B; p->device = device;
    // the kernel family: Normal closure; operator table with |kappa| > 4 terms (TME order 3: the 29-row layout); operator
    // table with the node tables of a joint likelihood; operator table
    const bool joint = model->n_factors == 1 && model->fac_component[0] == 2;
    p->launch = (model->trans_kind == MFS_ND_TRANS_GAUSSIAN) ? ke.launch_gauss
                : (model->n_terms > MFS_ND_TERMS) ? ke.launch_hi : joint ? ke.launch_joint : ke.launch;
    const size_t S = ke.S, DD = (size_t)model->extent * model->extent;
    const size_t ncoef = (size_t)(model->coef_batched ? B : 1) * n_rows * DD;
    const size_t nlik = (size_t)(model->lik_batched ? B : 1) * model->n_factors * MFS_MAX_LIK;
    const hipError_t e = upload_nd_tables(p, model->coef, ncoef, model->lik, nlik, inds, 3 * S * S);
    if (e != hipSuccess) {
        destroy_plan_nd(p, true);
        return fail(e == hipErrorOutOfMemory ? MFS_ENOMEM : MFS_EHIP, "mfs_plan_nd_create: %s", hipGetErrorString(e));
    }
    mfs::FilterNdArgs& a = p->args;
    fill_nd_args(a, p, model);
    a.stable = stable; a.n_terms_used = model->n_terms;
    // stable = 1: the completion on the register front end (a.stable = 1); MFS_ND_STABLE=dense keeps the LDS-tile form (2)
    if (stable) { const char* e = getenv("MFS_ND_STABLE"); a.stable = (e && strcmp(e, "dense") == 0) ? 2 : 1; }
    if (const char* e = getenv("MFS_ND_UPDATE")) {   // A/B switches, like MFS_SOLVER
        a.force_eigen = (strcmp(e, "eigen") == 0);
        a.joint_grid = (strcmp(e, "grid") == 0);
    }
    // true extents of each coefficient block (trailing zero rows / columns cut); the union over replicates when batched
    const size_t ntab = model->coef_batched ? (size_t)B : 1;
    for (int k = 0; k < n_rows; ++k) {
        int ea = 0, eb = 0;
        for (size_t r = 0; r < ntab; ++r) {
            const double* blk = model->coef + (r * n_rows + k) * DD;
            for (int i = 0; i < model->extent; ++i)
                for (int j = 0; j < model->extent; ++j)
                    if (blk[i * model->extent + j] != 0.0) { if (i + 1 > ea) ea = i + 1; if (j + 1 > eb) eb = j + 1; }
        }
        a.ext[k] = (ea == 0) ? 0 : (ea | (eb << 8));
    }
    *plan = p;
    return MFS_OK;
}

// one launch over the steps [t0, t1) of the plan's run; `carry` ([B][carry_doubles], or null for a single launch over [0, T))
// takes the state from one chunk to the next
static int plan_nd_launch(mfs_plan_nd* p, const double* d_m0, int m0_batched, const double* d_mean0, const double* d_scale0,
                          const double* d_ys, double* d_out_moments, double* d_out_means, double* d_out_scales,
                          double* d_out_nell, int32_t* d_out_first_nan, int t0, int t1, double* carry, hipStream_t stream) {
    mfs::FilterNdArgs a = p->args;
    a.m0 = d_m0; a.m0_batched = m0_batched; a.mean0 = d_mean0; a.scale0 = d_scale0; a.ys = d_ys;
    a.out_mom = d_out_moments;
    a.out_mean = (p->mode != MFS_MODE_RAW) ? d_out_means : nullptr;
    a.out_scale = (p->mode == MFS_MODE_SCALED) ? d_out_scales : nullptr;
    a.out_nell = d_out_nell; a.out_first_nan = d_out_first_nan;
    a.t_begin = t0; a.t_end = t1; a.carry = carry;
    const hipError_t e = p->launch(a, p->B, stream);
    if (e != hipSuccess) return fail(MFS_EHIP, "N-D kernel launch: %s", hipGetErrorString(e));
    return MFS_OK;
}

extern "C" int mfs_plan_nd_run(mfs_plan_nd* p, const double* d_m0, int m0_batched, const double* d_mean0,
                               const double* d_scale0, const double* d_ys, double* d_out_moments, double* d_out_means,
                               double* d_out_scales, double* d_out_nell, int32_t* d_out_first_nan, void* stream) {
    if (!p) return fail(MFS_EINVAL, "plan is NULL");
    if (p->B == 0) return MFS_OK;
    if (int rc = check_run_pointers(p->mode, d_m0, d_mean0, d_scale0, d_ys, d_out_nell, p->T, p->B)) return rc;
    HIP_TRY(hipSetDevice(p->device));
    return plan_nd_launch(p, d_m0, m0_batched, d_mean0, d_scale0, d_ys, d_out_moments, d_out_means, d_out_scales, d_out_nell,
                          d_out_first_nan, 0, p->T, nullptr, (hipStream_t)stream);
}

extern "C" int mfs_plan_nd_destroy(mfs_plan_nd* p) {
    if (p) destroy_plan_nd(p, false);
    return MFS_OK;
}

extern "C" int mfs_plan_nd_geometry(const mfs_plan_nd* p, int* threads_per_filter, int* grid, int* lds_bytes_per_block) {
    if (!p) return fail(MFS_EINVAL, "plan is NULL");
    if (threads_per_filter) *threads_per_filter = 256;
    if (grid) *grid = p->B;
    if (lds_bytes_per_block) *lds_bytes_per_block = mfs::g_nd_table[p->N].lds_bytes;
    return MFS_OK;
}

extern "C" int mfs_filter_nd(const mfs_model_nd* model, int mode, int N, int T, int B, int z,
                             const int32_t* multi_indices, const int32_t* inds, const double* m0, int m0_batched,
                             const double* mean0, const double* scale0, const double* ys, int stable,
                             double* out_moments, double* out_means, double* out_scales, double* out_nell,
                             int32_t* out_first_nan, int device, void* stream) {
    mfs_plan_nd* plan = nullptr;
    int rc = mfs_plan_nd_create(&plan, model, mode, N, T, B, z, multi_indices, inds, stable, device);
    if (rc != MFS_OK) return rc;
    struct Guard { mfs_plan_nd* p; ~Guard() { destroy_plan_nd(p, true); } } guard{plan};   // (every exit below is quiesced)
    if ((rc = check_run_pointers(mode, m0, mean0, scale0, ys, out_nell, T, B))) return rc;
    if (B == 0) return MFS_OK;
    const size_t Z = (size_t)z, nb = m0_batched ? B : 1, ny = (size_t)model->ny;
    double *d_m0 = nullptr, *d_mean0 = nullptr, *d_ys = nullptr, *d_mom = nullptr, *d_means = nullptr, *d_nell = nullptr,
           *d_scale0 = nullptr, *d_scales = nullptr;
    int32_t* d_fn = nullptr;
    mfs::Staging st(device, stream, true);
    st.alloc(&d_m0, nb * Z * 8);
    st.alloc(&d_mean0, nb * 2 * 8);
    st.alloc(&d_scale0, nb * 2 * 8);
    st.alloc(&d_ys, (size_t)B * T * ny * 8);
    if (out_moments) st.alloc(&d_mom, (size_t)B * T * Z * 8);
    if (out_means && mode != MFS_MODE_RAW) st.alloc(&d_means, (size_t)B * T * 2 * 8);
    if (out_scales && mode == MFS_MODE_SCALED) st.alloc(&d_scales, (size_t)B * T * 2 * 8);
    st.alloc(&d_nell, (size_t)B * 8);
    st.alloc(&d_fn, (size_t)B * 4);
    st.h2d(d_m0, m0, nb * Z * 8);
    if (mean0) st.h2d(d_mean0, mean0, nb * 2 * 8);
    if (scale0 && mode == MFS_MODE_SCALED) st.h2d(d_scale0, scale0, nb * 2 * 8);
    st.h2d(d_ys, ys, (size_t)B * T * ny * 8);
    // with the moments streamed out in chunks, the per-replicate state crosses the launches through a carry block, so the
    // bits are those of the single launch
    const int nchunks = host_chunks(device, T, B, Z, out_moments != nullptr);
    double* d_carry = nullptr;
    if (nchunks > 1) st.alloc(&d_carry, (size_t)B * mfs::g_nd_table[N].carry_doubles * 8);
    rc = mfs::run_streaming_out(st, T, B, nchunks, Z, out_moments, d_mom, [&](int t0, int t1) {
        return plan_nd_launch(plan, d_m0, m0_batched, d_mean0, d_scale0, d_ys, d_mom, d_means, d_scales, d_nell, d_fn, t0, t1,
                              d_carry, st.s);
    });
    if (rc == MFS_OK) {
        st.d2h(out_means, d_means, (size_t)B * T * 2 * 8);
        st.d2h(out_scales, d_scales, (size_t)B * T * 2 * 8);
        st.d2h(out_nell, d_nell, (size_t)B * 8);
        st.d2h(out_first_nan, d_fn, (size_t)B * 4);
    }
    return st.finish("mfs_filter_nd", rc);
}

// ---------------------------------------------------------------------------------------------------------------
// N-D filter, d = 3
// ---------------------------------------------------------------------------------------------------------------
struct mfs_plan_nd3 : NdPlanBase {
    // the kernel of the model, resolved at creation: `launch_joint` (with `joint`) if it has joint factors, else `launch`
    mfs::FilterNd3Launch launch = nullptr;
    mfs::FilterNd3JointLaunch launch_joint = nullptr;
    mfs::FilterNd3Args args;  // model part filled at create (device pointers), data pointers per run
    mfs::FilterNd3Joint joint;
    double* d_jcoef = nullptr;
    double* d_jpar = nullptr;
};

static void destroy_plan_nd3(mfs_plan_nd3* p, bool quiesced) {
    mfs::BlockPool<false>& pool = release_nd_tables(p, quiesced);
    pool.release(p->d_jcoef); pool.release(p->d_jpar);
    delete p;
}

// packed true extents of one [D][D][D] coefficient block over ntab tables `stride` doubles apart (0: all zero)
static int nd3_block_extents(const double* blk, size_t D, size_t ntab, size_t stride) {
    int ea = 0, eb = 0, ec = 0;
    for (size_t r = 0; r < ntab; ++r)
        for (size_t i = 0; i < D; ++i)
            for (size_t j = 0; j < D; ++j)
                for (size_t l = 0; l < D; ++l)
                    if (blk[r * stride + (i * D + j) * D + l] != 0.0) {
                        if ((int)i + 1 > ea) ea = (int)i + 1;
                        if ((int)j + 1 > eb) eb = (int)j + 1;
                        if ((int)l + 1 > ec) ec = (int)l + 1;
                    }
    return (ea == 0) ? 0 : (ea | (eb << 8) | (ec << 16));
}

// joint == nullptr: the model of mfs_plan_nd3_create (1..3 single-component factors, ny <= 3)
static int plan_nd3_create(mfs_plan_nd3** plan, const mfs_model_nd3* model, const mfs_joint_nd3* joint, int mode, int N, int T,
                           int B, int z, const int32_t* multi_indices, const int32_t* inds, int stable, int device) {
    if (!plan) return fail(MFS_EINVAL, "plan is NULL");
    *plan = nullptr;
    if (!model) return fail(MFS_EINVAL, "model is NULL");
    if (mode != MFS_MODE_RAW && mode != MFS_MODE_CENTRAL && mode != MFS_MODE_SCALED)
        return fail(MFS_EINVAL, "unknown moment mode %d", mode);
    if (N < MFS_ND3_MIN_N || N > MFS_ND3_MAX_N)
        return fail(MFS_EUNSUPPORTED, "N = %d outside [%d, %d] for d = 3", N, MFS_ND3_MIN_N, MFS_ND3_MAX_N);
    const mfs::Nd3Entry& ke = mfs::g_nd3_table[N];
    if (!ke.launch) return fail(MFS_EUNSUPPORTED, "no d = 3 kernel compiled for N = %d", N);
    if (model->trans_kind != MFS_ND_TRANS_OPERATOR && model->trans_kind != MFS_ND_TRANS_GAUSSIAN)
        return fail(MFS_EINVAL, "unknown N-D transition kind %d", model->trans_kind);
    if (model->n_terms != (model->trans_kind == MFS_ND_TRANS_GAUSSIAN ? MFS_ND3_GAUSS_TERMS : MFS_ND3_TERMS))
        return fail(MFS_EINVAL, "n_terms %d: the d = 3 tables carry %d operator terms or %d Normal-closure polynomials",
                    model->n_terms, MFS_ND3_TERMS, MFS_ND3_GAUSS_TERMS);
    if (z != ke.Z) return fail(MFS_EINVAL, "The size of multi_indices %d must match that of the moments %d.", z, ke.Z);
    if (model->extent < 1 || model->extent > MFS_ND3_MAX_EXTENT)
        return fail(MFS_EUNSUPPORTED, "coefficient extent %d outside [1, %d]", model->extent, MFS_ND3_MAX_EXTENT);
    const int min_factors = joint ? 0 : 1, max_ny = joint ? MFS_ND3_JOINT_MAX_NY : 3;
    if (model->n_factors < min_factors || model->n_factors > MFS_ND3_MAX_FACTORS)
        return fail(MFS_EINVAL, "n_factors %d outside [%d, %d]", model->n_factors, min_factors, MFS_ND3_MAX_FACTORS);
    if (model->ny < 1 || model->ny > max_ny) return fail(MFS_EINVAL, "ny %d outside [1, %d]", model->ny, max_ny);
    if (joint) {
        if (joint->n_joint < 1 || joint->n_joint > MFS_ND3_MAX_JOINT)
            return fail(MFS_EINVAL, "n_joint %d outside [1, %d]", joint->n_joint, MFS_ND3_MAX_JOINT);
        if (joint->extent < 1 || joint->extent > MFS_ND3_JOINT_MAX_EXTENT)
            return fail(MFS_EUNSUPPORTED, "joint polynomial extent %d outside [1, %d]", joint->extent, MFS_ND3_JOINT_MAX_EXTENT);
        for (int f = 0; f < joint->n_joint; ++f) {
            if (joint->kind[f] < 0 || joint->kind[f] > MFS_LIK_GAUSSIAN)
                return fail(MFS_EINVAL, "joint factor %d: kind %d is not Bernoulli-logistic, Poisson-softplus or Gaussian", f, joint->kind[f]);
            if (joint->link[f] < MFS_ND3_LINK_POLY || joint->link[f] > MFS_ND3_LINK_ATAN2_SQRT)
                return fail(MFS_EINVAL, "joint factor %d: unknown link %d", f, joint->link[f]);
            if (joint->ycol[f] < 0 || joint->ycol[f] >= model->ny)
                return fail(MFS_EINVAL, "joint factor %d: measurement column %d outside [0, ny = %d)", f, joint->ycol[f], model->ny);
        }
        if (!joint->coef || !joint->par) return fail(MFS_EINVAL, "NULL buffer");
    }
    for (int f = 0; f < model->n_factors; ++f) {
        if (model->fac_kind[f] == MFS_LIK_BEARING_GAUSSIAN)
            return fail(MFS_EUNSUPPORTED, "a likelihood of several state components is not supported at d = 3");
        if (model->fac_kind[f] < 0 || model->fac_kind[f] > MFS_LIK_GAUSSIAN || model->fac_n_par[f] < 1 ||
            model->fac_n_par[f] > MFS_MAX_LIK || model->fac_component[f] < 0 || model->fac_component[f] > 2 ||
            model->fac_ycol[f] < 0 || model->fac_ycol[f] >= model->ny)
            return fail(MFS_EINVAL, "bad description of likelihood factor %d", f);
    }
    if (T < 0 || B < 0) return fail(MFS_EINVAL, "negative T or B");
    if (!multi_indices || !inds || !model->coef || (model->n_factors > 0 && !model->lik)) return fail(MFS_EINVAL, "NULL buffer");
    const int S = ke.S;
    // the kernel derives a moment's multi-index from its position: insist on the graded-lex tables
    for (int zi = 0; zi < z; ++zi)
        for (int k = 0; k < 3; ++k)
            if (multi_indices[3 * zi + k] != mfs::nd3_exp(zi, k))
                return fail(MFS_EINVAL, "multi_indices is not the graded-lexicographic table of order 2N-1");
    for (int t = 0; t < 4; ++t)
        for (int i = 0; i < S; ++i)
            for (int j = 0; j < S; ++j) {
                const int want = mfs::nd3_index(mfs::nd3_exp(i, 0) + mfs::nd3_exp(j, 0) + (t == 1),
                                                mfs::nd3_exp(i, 1) + mfs::nd3_exp(j, 1) + (t == 2),
                                                mfs::nd3_exp(i, 2) + mfs::nd3_exp(j, 2) + (t == 3));
                if (inds[((size_t)t * S + i) * S + j] != want)
                    return fail(MFS_EUNSUPPORTED, "inds[%d][%d][%d] = %d is not the graded-lexicographic Gram / Hankel table (expected %d)",
                                t, i, j, inds[((size_t)t * S + i) * S + j], want);
            }
    HIP_TRY(hipSetDevice(device));
    mfs_plan_nd3* p = new (std::nothrow) mfs_plan_nd3();
    if (!p) return fail(MFS_ENOMEM, "out of host memory");
    p->mode = mode; p->N = N; p->T = T; p->B = B; p->device = device;
    const bool gauss = model->trans_kind == MFS_ND_TRANS_GAUSSIAN;
    if (joint) p->launch_joint = gauss ? ke.joint_gauss : ke.joint;
    else p->launch = gauss ? ke.launch_gauss : ke.launch;
    const size_t D = (size_t)model->extent, DDD = D * D * D;
    const size_t ncoef = (size_t)(model->coef_batched ? B : 1) * MFS_ND3_ROWS * DDD;
    const size_t nlik = (size_t)(model->lik_batched ? B : 1) * model->n_factors * MFS_MAX_LIK;
    hipError_t e = upload_nd_tables(p, model->coef, ncoef, model->lik, nlik, inds, (size_t)4 * S * S);
    mfs::BlockPool<false>& pool = mfs::device_state(device).device;
    const size_t E = joint ? (size_t)joint->extent : 0, jblk = 2 * E * E * E, jtab = joint ? (size_t)joint->n_joint * jblk : 0;
    const size_t njb = (joint && joint->batched) ? (size_t)B : 1;
    if (joint) {
        const size_t njpar = njb * joint->n_joint;
        if (e == hipSuccess) e = pool.acquire((void**)&p->d_jcoef, njb * jtab * 8);
        if (e == hipSuccess) e = pool.acquire((void**)&p->d_jpar, njpar * 8);
        if (e == hipSuccess && njb) e = hipMemcpy(p->d_jcoef, joint->coef, njb * jtab * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess && njb) e = hipMemcpy(p->d_jpar, joint->par, njpar * 8, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        destroy_plan_nd3(p, true);
        return fail(e == hipErrorOutOfMemory ? MFS_ENOMEM : MFS_EHIP, "mfs_plan_nd3_create: %s", hipGetErrorString(e));
    }
    mfs::FilterNd3Args& a = p->args;
    fill_nd_args(a, p, model);
    a.stable = stable ? 1 : 0; a.trans_kind = model->trans_kind;
    // true extents of each coefficient block (trailing zero planes cut); the union over replicates when batched
    const size_t ntab = model->coef_batched ? (size_t)B : 1;
    const int used_rows = gauss ? MFS_ND3_GAUSS_TERMS : MFS_ND3_ROWS;
    for (int k = 0; k < MFS_ND3_ROWS; ++k)
        a.ext[k] = (k < used_rows) ? nd3_block_extents(model->coef + (size_t)k * DDD, D, ntab, MFS_ND3_ROWS * DDD) : 0;
    mfs::FilterNd3Joint& jt = p->joint;
    memset(&jt, 0, sizeof(jt));
    if (joint) {
        jt.n = joint->n_joint; jt.E = joint->extent; jt.batched = joint->batched ? 1 : 0;
        for (int f = 0; f < joint->n_joint; ++f) {
            jt.kind[f] = joint->kind[f]; jt.link[f] = joint->link[f]; jt.ycol[f] = joint->ycol[f];
            for (int w = 0; w < 2; ++w)
                jt.ext[f][w] = nd3_block_extents(joint->coef + (size_t)f * jblk + (size_t)w * E * E * E, E, njb, jtab);
        }
        jt.coef = p->d_jcoef; jt.par = p->d_jpar;
    }
    *plan = p;
    return MFS_OK;
}

extern "C" int mfs_plan_nd3_create(mfs_plan_nd3** plan, const mfs_model_nd3* model, int mode, int N, int T, int B, int z,
                                   const int32_t* multi_indices, const int32_t* inds, int stable, int device) {
    return plan_nd3_create(plan, model, nullptr, mode, N, T, B, z, multi_indices, inds, stable, device);
}

extern "C" int mfs_plan_nd3_create_joint(mfs_plan_nd3** plan, const mfs_model_nd3* model, const mfs_joint_nd3* joint, int mode,
                                         int N, int T, int B, int z, const int32_t* multi_indices, const int32_t* inds,
                                         int stable, int device) {
    if (plan) *plan = nullptr;
    if (!joint) return fail(MFS_EINVAL, "joint is NULL (a model without joint factors goes through mfs_plan_nd3_create)");
    return plan_nd3_create(plan, model, joint, mode, N, T, B, z, multi_indices, inds, stable, device);
}

extern "C" int mfs_plan_nd3_run(mfs_plan_nd3* p, const double* d_m0, int m0_batched, const double* d_mean0,
                                const double* d_scale0, const double* d_ys, double* d_out_moments, double* d_out_means,
                                double* d_out_scales, double* d_out_nell, int32_t* d_out_first_nan, void* stream) {
    if (!p) return fail(MFS_EINVAL, "plan is NULL");
    if (p->B == 0) return MFS_OK;
    if (int rc = check_run_pointers(p->mode, d_m0, d_mean0, d_scale0, d_ys, d_out_nell, p->T, p->B)) return rc;
    HIP_TRY(hipSetDevice(p->device));
    mfs::FilterNd3Args a = p->args;
    a.m0 = d_m0; a.m0_batched = m0_batched; a.mean0 = d_mean0; a.scale0 = d_scale0; a.ys = d_ys;
    a.out_mom = d_out_moments;
    a.out_mean = (p->mode != MFS_MODE_RAW) ? d_out_means : nullptr;
    a.out_scale = (p->mode == MFS_MODE_SCALED) ? d_out_scales : nullptr;
    a.out_nell = d_out_nell; a.out_first_nan = d_out_first_nan;
    const hipError_t e = p->launch_joint ? p->launch_joint(a, p->joint, p->B, (hipStream_t)stream)
                                         : p->launch(a, p->B, (hipStream_t)stream);
    if (e != hipSuccess) return fail(MFS_EHIP, "d = 3 kernel launch: %s", hipGetErrorString(e));
    return MFS_OK;
}

extern "C" int mfs_plan_nd3_destroy(mfs_plan_nd3* p) {
    if (p) destroy_plan_nd3(p, false);
    return MFS_OK;
}

extern "C" int mfs_plan_nd3_geometry(const mfs_plan_nd3* p, int* threads_per_filter, int* grid, int* lds_bytes_per_block) {
    if (!p) return fail(MFS_EINVAL, "plan is NULL");
    if (threads_per_filter) *threads_per_filter = 256;
    if (grid) *grid = p->B;
    if (lds_bytes_per_block) *lds_bytes_per_block = mfs::g_nd3_table[p->N].lds_bytes;
    return MFS_OK;
}

static int filter_nd3(const mfs_model_nd3* model, const mfs_joint_nd3* joint, int mode, int N, int T, int B, int z,
                      const int32_t* multi_indices, const int32_t* inds, const double* m0, int m0_batched,
                      const double* mean0, const double* scale0, const double* ys, int stable,
                      double* out_moments, double* out_means, double* out_scales, double* out_nell,
                      int32_t* out_first_nan, int device, void* stream) {
    mfs_plan_nd3* plan = nullptr;
    int rc = plan_nd3_create(&plan, model, joint, mode, N, T, B, z, multi_indices, inds, stable, device);
    if (rc != MFS_OK) return rc;
    struct Guard { mfs_plan_nd3* p; ~Guard() { destroy_plan_nd3(p, true); } } guard{plan};   // (every exit below is quiesced)
    if ((rc = check_run_pointers(mode, m0, mean0, scale0, ys, out_nell, T, B))) return rc;
    if (B == 0) return MFS_OK;
    const size_t Z = (size_t)z, nb = m0_batched ? B : 1, ny = (size_t)model->ny;
    double *d_m0 = nullptr, *d_mean0 = nullptr, *d_scale0 = nullptr, *d_ys = nullptr, *d_mom = nullptr, *d_means = nullptr,
           *d_scales = nullptr, *d_nell = nullptr;
    int32_t* d_fn = nullptr;
    mfs::Staging st(device, stream, true);
    st.alloc(&d_m0, nb * Z * 8);
    st.alloc(&d_mean0, nb * 3 * 8);
    st.alloc(&d_scale0, nb * 3 * 8);
    st.alloc(&d_ys, (size_t)B * T * ny * 8 + 8);
    if (out_moments) st.alloc(&d_mom, (size_t)B * T * Z * 8 + 8);
    if (out_means && mode != MFS_MODE_RAW) st.alloc(&d_means, (size_t)B * T * 3 * 8 + 8);
    if (out_scales && mode == MFS_MODE_SCALED) st.alloc(&d_scales, (size_t)B * T * 3 * 8 + 8);
    st.alloc(&d_nell, (size_t)B * 8);
    st.alloc(&d_fn, (size_t)B * 4);
    st.h2d(d_m0, m0, nb * Z * 8);
    if (mean0 && mode != MFS_MODE_RAW) st.h2d(d_mean0, mean0, nb * 3 * 8);
    if (scale0 && mode == MFS_MODE_SCALED) st.h2d(d_scale0, scale0, nb * 3 * 8);
    st.h2d(d_ys, ys, (size_t)B * T * ny * 8);
    if (st.err == hipSuccess) {
        rc = mfs_plan_nd3_run(plan, d_m0, m0_batched, d_mean0, d_scale0, d_ys, d_mom, d_means, d_scales, d_nell, d_fn, st.s);
        if (rc == MFS_OK) {
            st.d2h(out_moments, d_mom, (size_t)B * T * Z * 8);
            st.d2h(out_means, d_means, (size_t)B * T * 3 * 8);
            st.d2h(out_scales, d_scales, (size_t)B * T * 3 * 8);
            st.d2h(out_nell, d_nell, (size_t)B * 8);
            st.d2h(out_first_nan, d_fn, (size_t)B * 4);
        }
    }
    return st.finish("mfs_filter_nd3", rc);
}

extern "C" int mfs_filter_nd3(const mfs_model_nd3* model, int mode, int N, int T, int B, int z,
                              const int32_t* multi_indices, const int32_t* inds, const double* m0, int m0_batched,
                              const double* mean0, const double* scale0, const double* ys, int stable,
                              double* out_moments, double* out_means, double* out_scales, double* out_nell,
                              int32_t* out_first_nan, int device, void* stream) {
    return filter_nd3(model, nullptr, mode, N, T, B, z, multi_indices, inds, m0, m0_batched, mean0, scale0, ys, stable,
                      out_moments, out_means, out_scales, out_nell, out_first_nan, device, stream);
}

extern "C" int mfs_filter_nd3_joint(const mfs_model_nd3* model, const mfs_joint_nd3* joint, int mode, int N, int T, int B, int z,
                                    const int32_t* multi_indices, const int32_t* inds, const double* m0, int m0_batched,
                                    const double* mean0, const double* scale0, const double* ys, int stable,
                                    double* out_moments, double* out_means, double* out_scales, double* out_nell,
                                    int32_t* out_first_nan, int device, void* stream) {
    if (!joint) return fail(MFS_EINVAL, "joint is NULL (a model without joint factors goes through mfs_filter_nd3)");
    return filter_nd3(model, joint, mode, N, T, B, z, multi_indices, inds, m0, m0_batched, mean0, scale0, ys, stable,
                      out_moments, out_means, out_scales, out_nell, out_first_nan, device, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// diagnostic: the kernels' elementary functions
// ---------------------------------------------------------------------------------------------------------------
extern "C" int mfs_elementary(int which, int n, const double* x, double* out, int device) {
    if (which < 0 || which > 2) return fail(MFS_EINVAL, "which = %d outside {0 exp, 1 tanh, 2 log}", which);
    if (n < 0) return fail(MFS_EINVAL, "negative n");
    if (n == 0) return MFS_OK;
    if (!x || !out) return fail(MFS_EINVAL, "NULL buffer");
    HIP_TRY(hipSetDevice(device));
    double *d_x = nullptr, *d_o = nullptr;
    mfs::Staging st(device, nullptr, false);   // null stream; this diagnostic copies synchronously
    st.alloc(&d_x, (size_t)n * 8);
    st.alloc(&d_o, (size_t)n * 8);
    if (st.err == hipSuccess) st.err = hipMemcpy(d_x, x, (size_t)n * 8, hipMemcpyHostToDevice);
    if (st.err == hipSuccess) st.err = mfs::launch_elementary(which, n, d_x, d_o, nullptr);
    if (st.err == hipSuccess) st.err = hipMemcpy(out, d_o, (size_t)n * 8, hipMemcpyDeviceToHost);
    (void)hipDeviceSynchronize();
    return st.finish("mfs_elementary", MFS_OK);
}

// ---------------------------------------------------------------------------------------------------------------
// characteristic function from moments, host pointers
// ---------------------------------------------------------------------------------------------------------------
extern "C" int mfs_characteristic_1d(int N, int count, const double* ms, const double* mean, const double* scale,
                                     int nz, const double* zs, double* out, int device, void* stream) {
    if (N < 2 || N > MFS_MAX_N) return fail(MFS_EUNSUPPORTED, "N = %d outside [2, %d]", N, MFS_MAX_N);
    if (count < 0 || nz < 0) return fail(MFS_EINVAL, "negative count or nz");
    if (count == 0 || nz == 0) return MFS_OK;
    if (!ms || !zs || !out) return fail(MFS_EINVAL, "NULL buffer");
    const int gi = mfs::default_group(N);
    mfs::Cf1dLaunch launch = mfs::g_fast[N][gi].cf;
    if (!launch) return fail(MFS_EUNSUPPORTED, "no kernel compiled for N = %d", N);
    HIP_TRY(hipSetDevice(device));
    const int fpb = 64 / mfs::group_lanes(gi);
    double *d_ms = nullptr, *d_mean = nullptr, *d_scale = nullptr, *d_zs = nullptr, *d_out = nullptr;
    mfs::Staging st(device, stream, false);   // on the caller's stream, null included
    st.alloc(&d_ms, (size_t)count * 2 * N * 8);
    st.alloc(&d_zs, (size_t)nz * 8);
    st.alloc(&d_out, (size_t)count * nz * 16);
    if (mean) st.alloc(&d_mean, (size_t)count * 8);
    if (scale) st.alloc(&d_scale, (size_t)count * 8);
    st.h2d(d_ms, ms, (size_t)count * 2 * N * 8);
    st.h2d(d_zs, zs, (size_t)nz * 8);
    if (mean) st.h2d(d_mean, mean, (size_t)count * 8);
    if (scale) st.h2d(d_scale, scale, (size_t)count * 8);
    if (st.err == hipSuccess) {
        mfs::Cf1dArgs a{count, nz, d_ms, d_mean, d_scale, d_zs, d_out};
        st.err = launch(a, (count + fpb - 1) / fpb, fpb * 2 * N * 8, st.s);
    }
    st.d2h(out, d_out, (size_t)count * nz * 16);
    return st.finish("mfs_characteristic_1d", MFS_OK);
}

// ---------------------------------------------------------------------------------------------------------------
// brute-force grid filter, host pointers (kernels: gridfilter_kernel.hpp)
// ---------------------------------------------------------------------------------------------------------------
extern "C" int mfs_grid_gemm_dev(int M, int N, int K, const double* d_A, const double* d_B, double* d_C, void* stream) {
    if (M <= 0 || N <= 0 || K <= 0 || M % mfs::kGridTile || N % mfs::kGridTile || K % mfs::kGridBK)
        return fail(MFS_EINVAL, "mfs_grid_gemm_dev: M = %d and N = %d must be positive multiples of %d, K = %d of %d", M, N,
                    mfs::kGridTile, K, mfs::kGridBK);
    if (!d_A || !d_B || !d_C || d_C == d_A || d_C == d_B) return fail(MFS_EINVAL, "mfs_grid_gemm_dev: NULL or aliased buffer");
    HIP_TRY(mfs::launch_grid_gemm(M, N, K, d_A, d_B, d_C, (hipStream_t)stream));
    return MFS_OK;
}

// trapezoid weights of jnp.trapz(., xs): w_0 = (x_1 - x_0) / 2, w_i = (x_{i+1} - x_{i-1}) / 2, w_{n-1} = (x_{n-1} - x_{n-2}) / 2
static std::vector<double> trapezoid_weights(int n, const double* xs) {
    std::vector<double> w((size_t)n);
    for (int i = 0; i < n; ++i) w[i] = 0.5 * (xs[i + 1 < n ? i + 1 : i] - xs[i > 0 ? i - 1 : i]);
    return w;
}

// what the two characteristic-function entries ask of their frequencies
static int check_grid_zs(const char* me, int nz, const double* zs, const double* out) {
    if (nz < 0) return fail(MFS_EINVAL, "%s: nz = %d < 0", me, nz);
    if (nz > 0 && (!zs || !out)) return fail(MFS_EINVAL, "%s: nz = %d needs zs and an output buffer", me, nz);
    if (nz > MFS_GRID_MAX_NZ) return fail(MFS_EUNSUPPORTED, "%s: nz = %d frequencies > %d", me, nz, MFS_GRID_MAX_NZ);
    for (int k = 0; k < nz; ++k)
        if (!std::isfinite(zs[k])) return fail(MFS_EINVAL, "%s: zs[%d] is not finite", me, k);
    return MFS_OK;
}

extern "C" int mfs_grid_filter_1d(int n, int T, int B, int substeps, int use_power, const double* xs, const double* trans_mean,
                                  const double* trans_sd, int lik_kind, int n_lik, const double* lik, int lik_batched,
                                  const double* init_ps, int init_batched, const double* ys, double* out_pdfs,
                                  double* out_means, double* out_vars, double* out_nell, int32_t* out_first_nan, int device,
                                  void* stream) {
    return mfs_grid_filter_1d_cf(n, T, B, substeps, use_power, xs, trans_mean, trans_sd, lik_kind, n_lik, lik, lik_batched,
                                 init_ps, init_batched, ys, 0, nullptr, out_pdfs, out_means, out_vars, nullptr, out_nell,
                                 out_first_nan, device, stream);
}

extern "C" int mfs_grid_filter_1d_cf(int n, int T, int B, int substeps, int use_power, const double* xs,
                                     const double* trans_mean, const double* trans_sd, int lik_kind, int n_lik,
                                     const double* lik, int lik_batched, const double* init_ps, int init_batched,
                                     const double* ys, int nz, const double* zs, double* out_pdfs, double* out_means,
                                     double* out_vars, double* out_cfs, double* out_nell, int32_t* out_first_nan, int device,
                                     void* stream) {
    if (n < 2 || T < 1 || B < 1) return fail(MFS_EINVAL, "mfs_grid_filter_1d: n = %d (>= 2), T = %d, B = %d (>= 1)", n, T, B);
    if (substeps < 1) return fail(MFS_EINVAL, "mfs_grid_filter_1d: substeps = %d < 1", substeps);
    if (n > MFS_GRID_MAX_N) return fail(MFS_EUNSUPPORTED, "mfs_grid_filter_1d: n = %d grid points > %d", n, MFS_GRID_MAX_N);
    if (lik_kind < MFS_LIK_BERNOULLI_LOGISTIC || lik_kind > MFS_LIK_GAUSSIAN)
        return fail(MFS_EINVAL, "mfs_grid_filter_1d: lik_kind %d is not a 1-D likelihood", lik_kind);
    if (n_lik < 1 || n_lik > MFS_MAX_LIK) return fail(MFS_EINVAL, "mfs_grid_filter_1d: n_lik %d outside [1, %d]", n_lik, MFS_MAX_LIK);
    if (!xs || !trans_mean || !trans_sd || !lik || !init_ps || !ys || !out_nell)
        return fail(MFS_EINVAL, "mfs_grid_filter_1d: xs / trans_mean / trans_sd / lik / init_ps / ys / out_nell must not be NULL");
    for (int i = 0; i < n; ++i) {
        if (!std::isfinite(xs[i]) || (i > 0 && !(xs[i] > xs[i - 1])))
            return fail(MFS_EINVAL, "mfs_grid_filter_1d: xs must be finite and strictly increasing (entry %d)", i);
        if (!std::isfinite(trans_sd[i]) || !(trans_sd[i] > 0.0))
            return fail(MFS_EINVAL, "mfs_grid_filter_1d: trans_sd[%d] = %g is not finite and > 0", i, trans_sd[i]);
    }
    if (const int rc = check_grid_zs("mfs_grid_filter_1d_cf", nz, zs, out_cfs)) return rc;
    HIP_TRY(hipSetDevice(device));
    const std::vector<double> w = trapezoid_weights(n, xs);

    const int n_pad = mfs::grid_pad(n), ldp = mfs::grid_pad(B);
    const size_t kk_bytes = (size_t)n_pad * n_pad * 8, p_bytes = (size_t)n_pad * ldp * 8, bt = (size_t)B * T;
    const size_t nb_lik = lik_batched ? (size_t)B : 1, nb_init = init_batched ? (size_t)B : 1;
    const bool power = use_power != 0 && substeps > 1;
    double *d_xs = nullptr, *d_m = nullptr, *d_sd = nullptr, *d_w = nullptr, *d_lik = nullptr, *d_init = nullptr, *d_ys = nullptr;
    double *d_K[3] = {nullptr, nullptr, nullptr}, *d_P[2] = {nullptr, nullptr};
    double *d_pdfs = nullptr, *d_means = nullptr, *d_vars = nullptr, *d_nell = nullptr;
    int32_t* d_fn = nullptr;
    mfs::Staging st(device, stream, true);
    st.alloc(&d_xs, (size_t)n * 8); st.alloc(&d_m, (size_t)n * 8); st.alloc(&d_sd, (size_t)n * 8); st.alloc(&d_w, (size_t)n * 8);
    st.alloc(&d_lik, nb_lik * n_lik * 8);
    st.alloc(&d_init, nb_init * n * 8);
    st.alloc(&d_ys, bt * 8);
    for (int k = 0; k < (power ? 3 : 1); ++k) st.alloc(&d_K[k], kk_bytes);
    st.alloc(&d_P[0], p_bytes); st.alloc(&d_P[1], p_bytes);
    if (out_pdfs) st.alloc(&d_pdfs, bt * n * 8);
    st.alloc(&d_means, bt * 8); st.alloc(&d_vars, bt * 8); st.alloc(&d_nell, (size_t)B * 8); st.alloc(&d_fn, (size_t)B * 4);
    // characteristic functions (nz > 0): the table, one product buffer and two output blocks of cf_S steps each, at most
    // 64 MB a block unless one step is larger (gridfilter_kernel.hpp)
    const int m_pad = mfs::grid_pad(nz);
    const size_t cf_step_bytes = (size_t)B * nz * 16;
    int cf_S = 0;
    double *d_zs = nullptr, *d_E = nullptr, *d_C = nullptr, *d_cf[2] = {nullptr, nullptr};
    if (nz > 0) {
        const size_t fit = ((size_t)64 << 20) / cf_step_bytes;
        cf_S = fit < 1 ? 1 : fit > (size_t)T ? T : (int)fit;
        st.alloc(&d_zs, (size_t)nz * 8);
        st.alloc(&d_E, (size_t)2 * m_pad * n_pad * 8);
        st.alloc(&d_C, (size_t)2 * m_pad * ldp * 8);
        st.alloc(&d_cf[0], cf_step_bytes * cf_S);
        if (cf_S < T) st.alloc(&d_cf[1], cf_step_bytes * cf_S);
        st.h2d(d_zs, zs, (size_t)nz * 8);
    }
    st.h2d(d_xs, xs, (size_t)n * 8); st.h2d(d_m, trans_mean, (size_t)n * 8); st.h2d(d_sd, trans_sd, (size_t)n * 8);
    st.h2d(d_w, w.data(), (size_t)n * 8);
    st.h2d(d_lik, lik, nb_lik * n_lik * 8);
    st.h2d(d_init, init_ps, nb_init * n * 8);
    st.h2d(d_ys, ys, bt * 8);
    if (st.err == hipSuccess) st.err = hipMemsetAsync(d_nell, 0, (size_t)B * 8, st.s);
    if (st.err == hipSuccess) st.err = hipMemsetAsync(d_fn, 0xff, (size_t)B * 4, st.s);   // -1
    if (st.err == hipSuccess) st.err = mfs::launch_grid_build_k(n, n_pad, d_xs, d_m, d_sd, d_w, d_K[0], st.s);
    if (st.err == hipSuccess) st.err = mfs::launch_grid_init_p(n, n_pad, B, ldp, d_init, init_batched != 0, d_P[0], st.s);
    if (nz > 0 && st.err == hipSuccess) st.err = mfs::launch_grid_cf_table(n, nz, n_pad, m_pad, 0, d_xs, d_w, d_zs, d_E, st.s);

    // the matrix of one measurement interval: K itself, or K^substeps by binary exponentiation over three buffers (at most
    // two are held by base and result at any time; launches on one stream are ordered, so a buffer given back is free).
    const double* d_M = d_K[0];
    if (power) {
        double* spare[3] = {d_K[1], d_K[2], nullptr};
        int nspare = 2;
        double *base = d_K[0], *res = nullptr;   // base = K^(2^bit); res = the product of the bases of the set bits so far
        for (int e = substeps; e > 0 && st.err == hipSuccess; e >>= 1) {
            if (e & 1) {
                if (!res) {
                    res = base;            // no copy: the squaring below leaves this buffer alone
                } else {
                    double* f = spare[--nspare];
                    st.err = mfs::launch_grid_gemm(n_pad, n_pad, n_pad, res, base, f, st.s);
                    spare[nspare++] = res;
                    res = f;
                }
            }
            if (e > 1 && st.err == hipSuccess) {
                double* f = spare[--nspare];
                st.err = mfs::launch_grid_gemm(n_pad, n_pad, n_pad, base, base, f, st.s);
                if (base != res) spare[nspare++] = base;
                base = f;
            }
        }
        d_M = res;
    }
    mfs::GridUpdateArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n; a.T = T; a.B = B; a.ldp = ldp; a.lik_kind = lik_kind; a.n_lik = n_lik; a.lik_batched = lik_batched != 0;
    a.xs = d_xs; a.w = d_w; a.lik = d_lik; a.ys = d_ys; a.out_pdfs = d_pdfs; a.out_means = d_means; a.out_vars = d_vars;
    a.nell = d_nell; a.first_nan = d_fn;
    // output block c (steps [c cf_S, ...)) to the host, on the copy stream once the block is filled: B rows of its steps'
    // pairs into out_cfs [B][T][nz][2]; one copy per replicate where the host pitch is beyond what a 2-D copy takes
    const bool cf_2d = nz > 0 && pitch_ok((size_t)T * nz * 16, device);
    auto drain_cf = [&](int c) {
        const int j = c & 1, t0 = c * cf_S, steps = (t0 + cf_S < T ? t0 + cf_S : T) - t0;
        const size_t row = (size_t)nz * 2;     // doubles per step and replicate
        if (st.err == hipSuccess) st.err = hipStreamWaitEvent(st.cx->copy, st.cx->ev[j], 0);
        if (cf_2d) {
            if (st.err == hipSuccess)
                st.err = hipMemcpy2DAsync(out_cfs + (size_t)t0 * row, (size_t)T * row * 8, d_cf[j], (size_t)cf_S * row * 8,
                                          (size_t)steps * row * 8, (size_t)B, hipMemcpyDeviceToHost, st.cx->copy);
        } else {
            for (int b = 0; b < B && st.err == hipSuccess; ++b)
                st.err = hipMemcpyAsync(out_cfs + ((size_t)b * T + t0) * row, d_cf[j] + (size_t)b * cf_S * row,
                                        (size_t)steps * row * 8, hipMemcpyDeviceToHost, st.cx->copy);
        }
        if (st.err == hipSuccess) st.err = hipEventRecord(st.cx->ev[2 + j], st.cx->copy);
    };
    const int reps = power ? 1 : substeps;
    int cur = 0;
    for (int t = 0; t < T && st.err == hipSuccess; ++t) {
        for (int r = 0; r < reps && st.err == hipSuccess; ++r) {
            st.err = mfs::launch_grid_gemm(n_pad, ldp, n_pad, d_M, d_P[cur], d_P[cur ^ 1], st.s);
            cur ^= 1;
        }
        a.t = t; a.P = d_P[cur];
        if (st.err == hipSuccess) st.err = mfs::launch_grid_update(a, st.s);
        if (nz == 0) continue;
        // cf of the posteriors of step t: one product with the table, stored at place t - t0 of output block c = t / cf_S.
        // Block c uses buffer c & 1; events 0, 1: buffer filled (compute stream), 2, 3: buffer drained (copy stream)
        const int c = t / cf_S, j = c & 1, slot = t - c * cf_S;
        if (slot == 0 && c >= 2 && st.err == hipSuccess) st.err = hipStreamWaitEvent(st.s, st.cx->ev[2 + j], 0);
        if (st.err == hipSuccess) st.err = mfs::launch_grid_gemm(2 * m_pad, ldp, n_pad, d_E, d_P[cur], d_C, st.s);
        if (st.err == hipSuccess) st.err = mfs::launch_grid_cf_store(nz, B, m_pad, ldp, cf_S, slot, d_C, d_fn, d_cf[j], st.s);
        if (slot == cf_S - 1 || t == T - 1) {
            if (st.err == hipSuccess) st.err = hipEventRecord(st.cx->ev[j], st.s);
            if (c >= 1) drain_cf(c - 1);      // one block behind: the copy of block c - 1 runs under the kernels of block c
            if (t == T - 1) drain_cf(c);
        }
    }
    st.d2h(out_pdfs, d_pdfs, bt * n * 8);
    st.d2h(out_means, d_means, bt * 8); st.d2h(out_vars, d_vars, bt * 8);
    st.d2h(out_nell, d_nell, (size_t)B * 8); st.d2h(out_first_nan, d_fn, (size_t)B * 4);
    return st.finish("mfs_grid_filter_1d", MFS_OK);
}

extern "C" int mfs_cf_from_pdf_1d(int n, int count, int nz, const double* xs, const double* zs, const double* ps, double* out,
                                  int device, void* stream) {
    const char* me = "mfs_cf_from_pdf_1d";
    if (n < 2 || count < 0) return fail(MFS_EINVAL, "%s: n = %d (>= 2), count = %d (>= 0)", me, n, count);
    if (n > MFS_GRID_MAX_N) return fail(MFS_EUNSUPPORTED, "%s: n = %d grid points > %d", me, n, MFS_GRID_MAX_N);
    if (const int rc = check_grid_zs(me, nz, zs, out)) return rc;
    if (count == 0 || nz == 0) return MFS_OK;
    if (!xs || !ps) return fail(MFS_EINVAL, "%s: xs / ps must not be NULL", me);
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(xs[i]) || (i > 0 && !(xs[i] > xs[i - 1])))
            return fail(MFS_EINVAL, "%s: xs must be finite and strictly increasing (entry %d)", me, i);
    HIP_TRY(hipSetDevice(device));
    const std::vector<double> w = trapezoid_weights(n, xs);

    // rows of densities per chunk: a multiple of the GEMM tile, sized so that a chunk's three buffers (densities, product,
    // pairs) stay within 64 MB; MFS_HOST_CHUNKS = c asks for c chunks instead
    const int n_pad = mfs::grid_pad(n), m_pad = mfs::grid_pad(nz);
    const size_t per_row = ((size_t)n_pad + 2 * (size_t)m_pad + 2 * (size_t)nz) * 8;
    size_t rows = ((size_t)64 << 20) / per_row;
    if (const char* e = getenv("MFS_HOST_CHUNKS")) {
        const int c = atoi(e);
        if (c >= 1) rows = ((size_t)count + c - 1) / c;
    }
    if (rows > (size_t)count) rows = (size_t)count;
    if (rows > 32768) rows = 32768;      // the store's grid has a row per block row
    const int R = mfs::grid_pad(rows < 1 ? 1 : (int)rows);

    double *d_xs = nullptr, *d_w = nullptr, *d_zs = nullptr, *d_E = nullptr, *d_ps = nullptr, *d_C = nullptr, *d_out = nullptr;
    mfs::Staging st(device, stream, true);
    st.alloc(&d_xs, (size_t)n * 8); st.alloc(&d_w, (size_t)n * 8); st.alloc(&d_zs, (size_t)nz * 8);
    st.alloc(&d_E, (size_t)n_pad * 2 * m_pad * 8);
    st.alloc(&d_ps, (size_t)R * n_pad * 8); st.alloc(&d_C, (size_t)R * 2 * m_pad * 8); st.alloc(&d_out, (size_t)R * nz * 16);
    st.h2d(d_xs, xs, (size_t)n * 8); st.h2d(d_w, w.data(), (size_t)n * 8); st.h2d(d_zs, zs, (size_t)nz * 8);
    if (st.err == hipSuccess) st.err = mfs::launch_grid_cf_table(n, nz, n_pad, m_pad, 1, d_xs, d_w, d_zs, d_E, st.s);
    // the padding of the density block (columns n .. n_pad, rows beyond a short last chunk) is zero; rows a chunk does not
    // overwrite keep an earlier chunk's densities, whose products are not stored
    if (st.err == hipSuccess) st.err = hipMemsetAsync(d_ps, 0, (size_t)R * n_pad * 8, st.s);
    for (int c0 = 0; c0 < count && st.err == hipSuccess; c0 += R) {
        const int rows_c = (c0 + R < count) ? R : count - c0;
        st.err = hipMemcpy2DAsync(d_ps, (size_t)n_pad * 8, ps + (size_t)c0 * n, (size_t)n * 8, (size_t)n * 8, (size_t)rows_c,
                                  hipMemcpyHostToDevice, st.s);
        if (st.err == hipSuccess) st.err = mfs::launch_grid_gemm(R, 2 * m_pad, n_pad, d_ps, d_E, d_C, st.s);
        if (st.err == hipSuccess) st.err = mfs::launch_grid_cf_store_rows(rows_c, nz, m_pad, d_C, d_out, st.s);
        st.d2h(out + (size_t)c0 * nz * 2, d_out, (size_t)rows_c * nz * 16);
    }
    return st.finish(me, MFS_OK);
}

// ---------------------------------------------------------------------------------------------------------------
// bootstrap particle filters, host pointers (kernels: particle_kernel.hpp for d = 1, particle_nd_kernel.hpp for d = 2).  The two
// entries share their argument check, their work buffers and the step driver below; each stages its own model and summaries
// ---------------------------------------------------------------------------------------------------------------
extern "C" int mfs_pf_draws(uint64_t seed, int t, int tag, int draw, int count, double* out_uniform, double* out_normal,
                            int device) {
    if (count < 0 || t < 0 || tag < 0 || draw < 0) return fail(MFS_EINVAL, "mfs_pf_draws: negative count, t, tag or draw");
    if (count == 0) return MFS_OK;
    if (!out_uniform || !out_normal) return fail(MFS_EINVAL, "mfs_pf_draws: NULL buffer");
    HIP_TRY(hipSetDevice(device));
    double *d_u = nullptr, *d_z = nullptr;
    mfs::Staging st(device, nullptr, true);
    st.alloc(&d_u, (size_t)count * 8);
    st.alloc(&d_z, (size_t)count * 8);
    if (st.err == hipSuccess) st.err = mfs::launch_pf_draws(seed, t, tag, draw, count, d_u, d_z, st.s);
    st.d2h(out_uniform, d_u, (size_t)count * 8);
    st.d2h(out_normal, d_z, (size_t)count * 8);
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

// The work buffers that do not depend on the state dimension: the seeds (uploaded), the weight scan, and what the `offsets`
// kernel takes -- the block totals, their offsets, the weight sums, nell (zeroed) and first_nan (-1) -- which is returned
static mfs::PfOffsetsArgs pf_work_buffers(mfs::Staging& st, int n, int B, const uint64_t* seeds, uint64_t** d_seeds,
                                          double** d_wscan) {
    mfs::PfOffsetsArgs o;
    memset(&o, 0, sizeof(o));
    o.n = n; o.B = B; o.nblk = mfs::pf_blocks(n);
    st.alloc(d_seeds, (size_t)B * 8); st.alloc(d_wscan, (size_t)B * n * 8);
    st.alloc(&o.wpart, (size_t)B * o.nblk * 8); st.alloc(&o.woffs, (size_t)B * o.nblk * 8); st.alloc(&o.wtot, (size_t)B * 8);
    st.alloc(&o.nell, (size_t)B * 8); st.alloc(&o.first_nan, (size_t)B * 4);
    st.h2d(*d_seeds, seeds, (size_t)B * 8);
    if (st.err == hipSuccess) st.err = hipMemsetAsync(o.nell, 0, (size_t)B * 8, st.s);
    if (st.err == hipSuccess) st.err = hipMemsetAsync(o.first_nan, 0xff, (size_t)B * 4, st.s);   // -1
    return o;
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

    const int nblk = mfs::pf_blocks(n), nseg = mfs::pf_segments(n), J1 = model->degree + 1;
    const size_t bn = (size_t)B * n, bt = (size_t)B * T;
    const size_t nb_coef = model->coef_batched ? (size_t)B : 1, nb_lik = model->lik_batched ? (size_t)B : 1;
    const size_t nb_init = init_batched ? (size_t)B : 1;
    double *d_coef = nullptr, *d_lik = nullptr, *d_ys = nullptr, *d_mix = nullptr, *d_init = nullptr, *d_zs = nullptr;
    uint64_t* d_seeds = nullptr;
    double *d_x = nullptr, *d_x2 = nullptr, *d_wscan = nullptr, *d_xpart = nullptr, *d_vpart = nullptr, *d_cfpart = nullptr;
    double *d_samples = nullptr, *d_means = nullptr, *d_vars = nullptr, *d_cfs = nullptr;
    mfs::Staging st(device, stream, true);
    st.alloc(&d_coef, nb_coef * 2 * J1 * 8); st.alloc(&d_lik, nb_lik * model->n_lik * 8); st.alloc(&d_ys, bt * 8);
    mfs::PfOffsetsArgs o = pf_work_buffers(st, n, B, seeds, &d_seeds, &d_wscan);
    if (n_mix > 0) st.alloc(&d_mix, (size_t)3 * n_mix * 8); else st.alloc(&d_init, nb_init * n * 8);
    if (nz > 0) st.alloc(&d_zs, (size_t)nz * 8);
    st.alloc(&d_x, bn * 8); st.alloc(&d_x2, bn * 8);
    st.alloc(&d_xpart, (size_t)B * nblk * 8); st.alloc(&d_vpart, (size_t)B * nseg * 8);
    if (nz > 0) st.alloc(&d_cfpart, (size_t)B * nseg * nz * 16);
    if (out_samples) st.alloc(&d_samples, bt * n * 8);
    st.alloc(&d_means, bt * 8); st.alloc(&d_vars, bt * 8);
    if (nz > 0) st.alloc(&d_cfs, bt * nz * 16);
    st.h2d(d_coef, model->coef, nb_coef * 2 * J1 * 8); st.h2d(d_lik, model->lik, nb_lik * model->n_lik * 8);
    st.h2d(d_ys, ys, bt * 8);
    if (n_mix > 0) {
        st.h2d(d_mix, mix_cumw, (size_t)n_mix * 8); st.h2d(d_mix + n_mix, mix_mean, (size_t)n_mix * 8);
        st.h2d(d_mix + 2 * n_mix, mix_var, (size_t)n_mix * 8);
    } else {
        st.h2d(d_init, init_samples, nb_init * n * 8);
    }
    if (nz > 0) st.h2d(d_zs, zs, (size_t)nz * 8);

    mfs::PfArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n; a.T = T; a.B = B; a.nblk = nblk; a.nseg = nseg; a.resampling = resampling;
    a.umap = model->umap; a.degree = model->degree; a.coef_batched = model->coef_batched != 0; a.lik_kind = model->lik_kind;
    a.n_lik = model->n_lik; a.lik_batched = model->lik_batched != 0; a.mean_x_coef = model->mean_x_coef;
    a.coef = d_coef; a.lik = d_lik; a.ys = d_ys; a.seeds = d_seeds;
    a.n_mix = n_mix; a.init_batched = init_batched != 0;
    if (n_mix > 0) { a.mix_cumw = d_mix; a.mix_mean = d_mix + n_mix; a.mix_var = d_mix + 2 * n_mix; }
    a.init = d_init; a.nz = nz; a.z_uniform = z_uniform; a.dz = dz; a.zs = d_zs;
    a.x = d_x; a.x2 = d_x2; a.wscan = d_wscan; a.wpart = o.wpart; a.woffs = o.woffs; a.wtot = o.wtot; a.xpart = d_xpart;
    a.vpart = d_vpart; a.cfpart = d_cfpart; a.out_samples = d_samples; a.out_means = d_means; a.out_vars = d_vars;
    a.out_cfs = d_cfs;
    if (st.err == hipSuccess) st.err = mfs::launch_pf_init(a, st.s);
    pf_run_steps(st, T, [&](int t) { a.t = o.t = t; },
                 [&](int k) {
                     return k == 0 ? mfs::launch_pf_propagate(a, st.s) : k == 1 ? mfs::launch_pf_offsets(o, st.s)
                          : k == 2 ? mfs::launch_pf_resample(a, st.s) : k == 3 ? mfs::launch_pf_cf(a, st.s)
                                                                               : mfs::launch_pf_finalize(a, st.s);
                 },
                 [&] { std::swap(a.x, a.x2); });   // the resampled particles are the next step's
    st.d2h(out_samples, d_samples, bt * n * 8);
    st.d2h(out_means, d_means, bt * 8); st.d2h(out_vars, d_vars, bt * 8);
    st.d2h(out_cfs, d_cfs, bt * nz * 16);
    st.d2h(out_nell, o.nell, (size_t)B * 8); st.d2h(out_first_nan, o.first_nan, (size_t)B * 4);
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

    const int nblk = mfs::pf_blocks(n), nseg = mfs::pf_segments(n), ny = model->ny, nf = model->n_factors;
    const size_t table = (size_t)MFS_ND_TABLE_ROWS(model->n_terms) * model->extent * model->extent;
    const size_t bn = (size_t)B * n, bt = (size_t)B * T;
    const size_t nb_coef = model->coef_batched ? (size_t)B : 1, nb_lik = model->lik_batched ? (size_t)B : 1;
    const size_t nb_init = init_batched ? (size_t)B : 1;
    double *d_coef = nullptr, *d_lik = nullptr, *d_ys = nullptr, *d_mix = nullptr, *d_init = nullptr;
    uint64_t* d_seeds = nullptr;
    double *d_x = nullptr, *d_x2 = nullptr, *d_wscan = nullptr, *d_xpart = nullptr, *d_cpart = nullptr;
    double *d_samples = nullptr, *d_means = nullptr, *d_covs = nullptr;
    mfs::Staging st(device, stream, true);
    st.alloc(&d_coef, nb_coef * table * 8); st.alloc(&d_lik, nb_lik * nf * MFS_MAX_LIK * 8); st.alloc(&d_ys, bt * ny * 8);
    mfs::PfOffsetsArgs o = pf_work_buffers(st, n, B, seeds, &d_seeds, &d_wscan);
    if (n_mix > 0) st.alloc(&d_mix, (size_t)7 * n_mix * 8); else st.alloc(&d_init, nb_init * n * 16);
    st.alloc(&d_x, bn * 16); st.alloc(&d_x2, bn * 16);
    st.alloc(&d_xpart, (size_t)B * nblk * 16); st.alloc(&d_cpart, (size_t)B * nseg * 24);
    if (out_samples) st.alloc(&d_samples, bt * n * 16);
    st.alloc(&d_means, bt * 16); st.alloc(&d_covs, bt * 32);
    st.h2d(d_coef, model->coef, nb_coef * table * 8); st.h2d(d_lik, model->lik, nb_lik * nf * MFS_MAX_LIK * 8);
    st.h2d(d_ys, ys, bt * ny * 8);
    if (n_mix > 0) {
        st.h2d(d_mix, mix_cumw, (size_t)n_mix * 8); st.h2d(d_mix + n_mix, mix_mean, (size_t)n_mix * 16);
        st.h2d(d_mix + 3 * n_mix, mix_chol, (size_t)n_mix * 32);
    } else {
        st.h2d(d_init, init_samples, nb_init * n * 16);
    }

    mfs::PfNdArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n; a.T = T; a.B = B; a.nblk = nblk; a.nseg = nseg; a.resampling = resampling;
    a.extent = model->extent; a.coef_stride = (int)table; a.coef_batched = model->coef_batched != 0;
    a.n_factors = nf; a.ny = ny; a.lik_batched = model->lik_batched != 0;
    for (int f = 0; f < nf; ++f) {
        a.fac_kind[f] = model->fac_kind[f]; a.fac_component[f] = model->fac_component[f]; a.fac_ycol[f] = model->fac_ycol[f];
    }
    a.coef = d_coef; a.lik = d_lik; a.ys = d_ys; a.seeds = d_seeds;
    a.n_mix = n_mix; a.init_batched = init_batched != 0;
    if (n_mix > 0) { a.mix_cumw = d_mix; a.mix_mean = d_mix + n_mix; a.mix_chol = d_mix + 3 * n_mix; }
    a.init = d_init;
    a.x = d_x; a.x2 = d_x2; a.wscan = d_wscan; a.wpart = o.wpart; a.woffs = o.woffs; a.wtot = o.wtot; a.xpart = d_xpart;
    a.cpart = d_cpart; a.out_samples = d_samples; a.out_means = d_means; a.out_covs = d_covs;
    if (st.err == hipSuccess) st.err = mfs::launch_pfnd_init(a, st.s);
    pf_run_steps(st, T, [&](int t) { a.t = o.t = t; },
                 [&](int k) {
                     return k == 0 ? mfs::launch_pfnd_propagate(a, st.s) : k == 1 ? mfs::launch_pf_offsets(o, st.s)
                          : k == 2 ? mfs::launch_pfnd_resample(a, st.s) : k == 3 ? mfs::launch_pfnd_cov(a, st.s)
                                                                                 : mfs::launch_pfnd_finalize(a, st.s);
                 },
                 [&] { std::swap(a.x, a.x2); });   // the resampled particles are the next step's
    st.d2h(out_samples, d_samples, bt * n * 16);
    st.d2h(out_means, d_means, bt * 16); st.d2h(out_covs, d_covs, bt * 32);
    st.d2h(out_nell, o.nell, (size_t)B * 8); st.d2h(out_first_nan, o.first_nan, (size_t)B * 4);
    return st.finish(me, MFS_OK);
}

// ---------------------------------------------------------------------------------------------------------------
// Gaussian filters: sigma-point filter and EKF, host pointers (kernels: gaussfilter_kernel.hpp)
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
    double *d_coef = nullptr, *d_lik = nullptr, *d_xi = nullptr, *d_w = nullptr, *d_m0 = nullptr, *d_P0 = nullptr, *d_ys = nullptr;
    double *d_means = nullptr, *d_covs = nullptr, *d_nells = nullptr;
    int32_t* d_fn = nullptr;
    mfs::Staging st(device, stream, true);
    st.alloc(&d_coef, coef_doubles * 8); st.alloc(&d_lik, lik_doubles * 8);
    if (np) { st.alloc(&d_xi, np * d * 8); st.alloc(&d_w, np * 8); }
    st.alloc(&d_m0, nb_init * d * 8); st.alloc(&d_P0, nb_init * d * d * 8); st.alloc(&d_ys, bt * 8);
    if (out_means) st.alloc(&d_means, bt * d * 8);
    if (out_covs) st.alloc(&d_covs, bt * d * d * 8);
    st.alloc(&d_nells, bt * 8);
    if (out_first_nan) st.alloc(&d_fn, (size_t)B * 4);
    st.h2d(d_coef, coef, coef_doubles * 8); st.h2d(d_lik, lik, lik_doubles * 8);
    if (np) { st.h2d(d_xi, xi, np * d * 8); st.h2d(d_w, w, np * 8); }
    st.h2d(d_m0, m0, nb_init * d * 8); st.h2d(d_P0, P0, nb_init * d * d * 8); st.h2d(d_ys, ys, bt * 8);
    a.coef = d_coef; a.lik = d_lik; a.xi = d_xi; a.w = d_w; a.m0 = d_m0; a.P0 = d_P0; a.ys = d_ys;
    a.out_means = d_means; a.out_covs = d_covs; a.out_nells = d_nells; a.out_first_nan = d_fn;
    if (st.err == hipSuccess) st.err = mfs::launch_gauss_filter(a, st.s);
    st.d2h(out_means, d_means, bt * d * 8); st.d2h(out_covs, d_covs, bt * d * d * 8);
    st.d2h(out_nells, d_nells, bt * 8); st.d2h(out_first_nan, d_fn, (size_t)B * 4);
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
    a.umap = model->umap; a.degree = model->degree; a.coef_batched = model->coef_batched != 0; a.lik_kind = model->lik_kind;
    a.n_lik = model->n_lik; a.lik_batched = model->lik_batched != 0; a.mean_x_coef = model->mean_x_coef;
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
