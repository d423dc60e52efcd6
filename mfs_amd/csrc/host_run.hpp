// host_run.hpp -- what the host units (capi*.hip) share beyond the registry and the staging: the HIP error macro, the checks on a
// run's data pointers, the chunking of a streamed run, and the description of a moment-filter run (its nine data pointers),
// staged from host pointers or taken from device pointers, and copied into any of the filters' argument structs.  Host-only code.
#pragma once
#include <cstdlib>

#include "registry.hpp"
#include "staging.hpp"

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return mfs::fail(MFS_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace mfs {

// what every run needs of its data pointers, device or host (ys only where there is a measurement to read)
static inline int check_run_pointers(int mode, const double* m0, const double* mean0, const double* scale0, const double* ys,
                                     const double* out_nell, int T, int B) {
    if (!m0 || !out_nell || (T > 0 && B > 0 && !ys)) return fail(MFS_EINVAL, "m0 / ys / out_nell must not be NULL");
    if (mode != MFS_MODE_RAW && !mean0) return fail(MFS_EINVAL, "mean0 is required in central and scaled modes");
    if (mode == MFS_MODE_SCALED && !scale0) return fail(MFS_EINVAL, "scale0 is required in scaled mode");
    return MFS_OK;
}

// hipMemcpy2DAsync takes a pitch: a row of T x (moments per step) x 8 bytes beyond the runtime's limit (runs of ~1e6 steps and
// more) would fail the whole call, so such runs go out in one linear copy instead (no copy / compute overlap)
static inline bool pitch_ok(size_t pitch_bytes, int device) {
    int maxp = 0;
    if (hipDeviceGetAttribute(&maxp, hipDeviceAttributeMaxPitch, device) != hipSuccess || maxp <= 0) return pitch_bytes < ((size_t)1 << 31);
    return pitch_bytes <= (size_t)maxp;
}

// How many T-chunks a host entry splits a run into when the moments ([B][T][width] doubles) are streamed out
// (run_streaming_out): one per 32 MB of them, at most 16.  MFS_HOST_CHUNKS overrides (1 = one launch, copies afterwards).
static inline int host_chunks(int device, int T, int B, size_t width, bool out_moments) {
    if (B <= 0 || T <= 0 || !pitch_ok((size_t)T * width * 8, device)) return 1;
    int n = out_moments ? (int)((size_t)B * T * width * 8 / ((size_t)32 << 20)) : 0;
    if (const char* e = getenv("MFS_HOST_CHUNKS")) n = atoi(e);
    if (n > 16) n = 16;
    if (n > T) n = T;
    return n < 1 ? 1 : n;
}

// The data of one moment-filter run, 1-D or N-D: device pointers.  An output the caller does not want is null.
struct FilterRun {
    const double* m0;
    int m0_batched;
    const double* mean0;
    const double* scale0;
    const double* ys;
    double* out_mom;
    double* out_mean;
    double* out_scale;
    double* out_nell;
    int32_t* out_first_nan;
};

// The run of a host-pointer entry: `nb` initial states of `width` moments, means and scales of `d` components, ys [B][T][ny].
// The moments are leased but not recorded (run_streaming_out copies them); st.download() brings the other outputs back in the
// order means, scales, nell, first_nan.  No kernel reads mean0 in raw mode or scale0 outside scaled mode: mean0 is uploaded
// whenever it is given, scale0 in scaled mode, and both blocks exist in every mode.  `pad` bytes are added to the leases of ys
// and of the [B][T] outputs (the d = 3 entries').
static inline FilterRun stage_filter_run(Staging& st, int mode, int B, int T, size_t nb, size_t width, size_t d, size_t ny,
                                         size_t pad, const double* m0, int m0_batched, const double* mean0, const double* scale0,
                                         const double* ys, double* out_moments, double* out_means, double* out_scales,
                                         double* out_nell, int32_t* out_first_nan) {
    const size_t bt = (size_t)B * T;
    FilterRun r;
    r.m0 = st.in(m0, nb * width * 8);
    r.m0_batched = m0_batched;
    r.mean0 = st.in(mean0, nb * d * 8);
    r.scale0 = st.in(mode == MFS_MODE_SCALED ? scale0 : nullptr, nb * d * 8);
    r.ys = st.in(ys, bt * ny * 8, pad);
    r.out_mom = st.out(out_moments, bt * width * 8, pad, Staging::kStreamed);
    r.out_mean = st.out(mode != MFS_MODE_RAW ? out_means : nullptr, bt * d * 8, pad);
    r.out_scale = st.out(mode == MFS_MODE_SCALED ? out_scales : nullptr, bt * d * 8, pad);
    r.out_nell = st.out(out_nell, (size_t)B * 8);
    r.out_first_nan = st.out(out_first_nan, (size_t)B * 4, 0, Staging::kAlways);
    return r;
}

// A run into the kernel arguments (Filter1dArgs, FilterNdArgs, FilterNd3Args name these fields alike): the one place that
// does it.  Means are written outside raw mode only, scales in scaled mode only, whatever the caller passed.
template <typename Args>
void set_run(Args& a, int mode, const FilterRun& r) {
    a.m0 = r.m0; a.m0_batched = r.m0_batched; a.mean0 = r.mean0; a.scale0 = r.scale0; a.ys = r.ys;
    a.out_mom = r.out_mom;
    a.out_mean = (mode != MFS_MODE_RAW) ? r.out_mean : nullptr;
    a.out_scale = (mode == MFS_MODE_SCALED) ? r.out_scale : nullptr;
    a.out_nell = r.out_nell; a.out_first_nan = r.out_first_nan;
}

}  // namespace mfs
