// staging.hpp -- the device staging of one host-pointer call (the capi*.hip units): blocks leased from the pool (pool.hpp), inputs
// uploaded as they are leased, outputs recorded as they are leased and downloaded together, and the closing synchronisation,
// with one sticky hipError_t: after the first failure every later step is a no-op, and finish() reports it.  Host-only code.
#pragma once
#include "../../include/mfs_hip.h"
#include "pool.hpp"

namespace mfs {

int fail(int code, const char* fmt, ...);   // capi.hip: sets mfs_last_error(), returns `code`

class Staging {
public:
    hipError_t err = hipSuccess;
    hipStream_t s = nullptr;        // where the call's copies and launches go
    CallContext* cx = nullptr;      // with_context only: s = the caller's stream if it gave one, else cx->compute

    // how out() treats a block: kStreamed -- leased, not recorded (the entry copies it out itself, e.g. run_streaming_out);
    // kAlways -- leased even without a host pointer (the kernel writes it whether the caller wants it or not)
    enum : unsigned { kStreamed = 1, kAlways = 2 };
    static constexpr int kMaxOutputs = 6;   // the 1-D particle filter's: samples, means, variances, cfs, nell, first_nan

    // with_context = false: the call runs on the caller's stream as it is (null included)
    Staging(int device, void* stream, bool with_context) : s((hipStream_t)stream), lease_(device) {
        if (with_context && (err = lease_.context(&cx)) == hipSuccess && !s) s = cx->compute;
    }
    // a block and nothing copied: work space, or a block that is filled from several host arrays (h2d) or zeroed on the device
    template <typename T = double>
    T* work(size_t bytes) {
        T* d = nullptr;
        if (err == hipSuccess) err = lease_.device_block(&d, bytes);
        return d;
    }
    // an input: a block of bytes + pad, and the upload of `bytes` where the caller gave the array
    template <typename T>
    T* in(const T* h, size_t bytes, size_t pad = 0) {
        T* d = work<T>(bytes + pad);
        if (h) h2d(d, h, bytes);
        return d;
    }
    // an output: null when the caller does not want it (but see kAlways); else a block of bytes + pad, whose first `bytes`
    // download() copies to `h`
    template <typename T>
    T* out(T* h, size_t bytes, size_t pad = 0, unsigned how = 0) {
        if (!h && !(how & kAlways)) return nullptr;
        T* d = work<T>(bytes + pad);
        if (h && !(how & kStreamed) && err == hipSuccess) {
            if (n_out_ == kMaxOutputs) err = hipErrorInvalidValue;     // (a new entry with more outputs: raise kMaxOutputs)
            else outs_[n_out_++] = Output{h, d, bytes};
        }
        return d;
    }
    // the recorded outputs, in the order they were recorded
    void download() {
        for (int k = 0; k < n_out_; ++k) d2h(outs_[k].h, outs_[k].d, outs_[k].bytes);
    }
    void h2d(void* d, const void* h, size_t bytes) {
        if (err == hipSuccess && bytes) err = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s);
    }
    // (an output the caller did not ask for has a null `h`, and then no device block either)
    void d2h(void* h, const void* d, size_t bytes) {
        if (err == hipSuccess && h && d && bytes) err = hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s);
    }
    // Quiesces the streams whatever happened before -- the pool blocks go back when this object unwinds -- and gives the
    // call's return code: `rc` if that is a failure, else the first HIP error, else MFS_OK.
    int finish(const char* name, int rc) {
        const hipError_t es = hipStreamSynchronize(s), ec = cx ? hipStreamSynchronize(cx->copy) : hipSuccess;
        if (rc != MFS_OK) return rc;
        if (err == hipSuccess) err = (es != hipSuccess) ? es : ec;
        if (err == hipSuccess) return MFS_OK;
        return fail(err == hipErrorOutOfMemory ? MFS_ENOMEM : MFS_EHIP, "%s: %s", name, hipGetErrorString(err));
    }

private:
    struct Output { void* h; const void* d; size_t bytes; };
    Lease lease_;
    Output outs_[kMaxOutputs];
    int n_out_ = 0;
};

// A run of T steps whose moments ([B][T][width] doubles, on the device and at the host) are streamed out: the run is cut
// into `nchunks` launches on st.s, and while the kernel of chunk k + 1 runs, chunk k's slice travels to the host on the copy
// stream (2-D copy: B rows of chunk x width doubles), released by an event.  launch(t0, t1) enqueues the steps [t0, t1) and
// returns an MFS code.  nchunks <= 1: one launch over [0, T), the copy after it.
template <typename Launch>
int run_streaming_out(Staging& st, int T, int B, int nchunks, size_t width, double* out_moments, const double* d_mom,
                      Launch&& launch) {
    if (st.err != hipSuccess) return MFS_OK;
    if (nchunks <= 1) {
        const int rc = launch(0, T);
        if (rc == MFS_OK) st.d2h(out_moments, d_mom, (size_t)B * T * width * 8);
        return rc;
    }
    const int chunk = (T + nchunks - 1) / nchunks;
    const size_t pitch = (size_t)T * width * 8;
    for (int k = 0, t0 = 0; t0 < T && st.err == hipSuccess; ++k, t0 += chunk) {
        const int t1 = (t0 + chunk < T) ? t0 + chunk : T;
        if (const int rc = launch(t0, t1)) return rc;
        st.err = hipEventRecord(st.cx->ev[k], st.s);
        if (st.err == hipSuccess) st.err = hipStreamWaitEvent(st.cx->copy, st.cx->ev[k], 0);
        if (st.err == hipSuccess && out_moments)
            st.err = hipMemcpy2DAsync(out_moments + (size_t)t0 * width, pitch, d_mom + (size_t)t0 * width, pitch,
                                      (size_t)(t1 - t0) * width * 8, (size_t)B, hipMemcpyDeviceToHost, st.cx->copy);
    }
    return MFS_OK;
}

}  // namespace mfs
