// capi.hip -- the core of the C ABI of libmfs_hip.so (include/mfs_hip.h): the last-error string, the runtime wrappers, the pool
// entries, the RCCL loader and the device-math diagnostics.  The filter families are units of their own: capi_1d.hip,
// capi_nd.hip, capi_grid.hip, capi_classical.hip.  No compute lives in any of them and no kernel header is included: launchers
// and argument structs come from registry.hpp, what the units share on the host from host_run.hpp.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <dlfcn.h>
#include <mutex>
#include <string>

#include "host_run.hpp"

namespace mfs {
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

using mfs::fail;

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
int mfs_memcpy_d2d(void* dst, const void* src, uint64_t bytes, void* stream) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
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

// ---------------------------------------------------------------------------------------------------------------
// diagnostic: the kernels' elementary functions
// ---------------------------------------------------------------------------------------------------------------
int mfs_elementary(int which, int n, const double* x, double* out, int device) {
    if (which < 0 || which > 2) return fail(MFS_EINVAL, "which = %d outside {0 exp, 1 tanh, 2 log}", which);
    if (n < 0) return fail(MFS_EINVAL, "negative n");
    if (n == 0) return MFS_OK;
    if (!x || !out) return fail(MFS_EINVAL, "NULL buffer");
    HIP_TRY(hipSetDevice(device));
    mfs::Staging st(device, nullptr, false);   // null stream; this diagnostic copies synchronously
    double *d_x = st.work((size_t)n * 8), *d_o = st.work((size_t)n * 8);
    if (st.err == hipSuccess) st.err = hipMemcpy(d_x, x, (size_t)n * 8, hipMemcpyHostToDevice);
    if (st.err == hipSuccess) st.err = mfs::launch_elementary(which, n, d_x, d_o, nullptr);
    if (st.err == hipSuccess) st.err = hipMemcpy(out, d_o, (size_t)n * 8, hipMemcpyDeviceToHost);
    (void)hipDeviceSynchronize();
    return st.finish("mfs_elementary", MFS_OK);
}

// diagnostic: the shared device math and the likelihood forms, one routine per call
int mfs_device_math(int fn, int n, int n_in, const double* in, int n_out, double* out, int device) {
    const mfs::DeviceMathShape shape = mfs::device_math_shape(fn);
    if (shape.n_in == 0) return fail(MFS_EINVAL, "mfs_device_math: fn = %d outside [0, %d)", fn, MFS_DM_COUNT);
    if (n <= 0) return fail(MFS_EINVAL, "mfs_device_math: n = %d (>= 1)", n);
    if (n_in != shape.n_in || n_out != shape.n_out)
        return fail(MFS_EINVAL, "mfs_device_math: fn = %d takes n_in = %d, n_out = %d, got %d, %d", fn, shape.n_in, shape.n_out,
                    n_in, n_out);
    if (!in || !out) return fail(MFS_EINVAL, "mfs_device_math: NULL buffer");
    HIP_TRY(hipSetDevice(device));
    mfs::Staging st(device, nullptr, true);
    const double* d_in = st.in(in, (size_t)n_in * n * 8);
    double* d_out = st.out(out, (size_t)n_out * n * 8);
    if (st.err == hipSuccess) st.err = mfs::launch_device_math(fn, n, d_in, d_out, st.s);
    st.download();
    return st.finish("mfs_device_math", MFS_OK);
}

}  // extern "C"
