// capi_grid.hip -- the brute-force grid filter of the C ABI (include/mfs_hip.h), host pointers: the filter with and without
// characteristic functions, the characteristic function of given densities, and the device GEMM (kernels:
// gridfilter_kernel.hpp, reached through registry.hpp only).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "host_run.hpp"

using mfs::fail;

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
    mfs::Staging st(device, stream, true);
    const size_t n8 = (size_t)n * 8;
    const double *d_xs = st.in(xs, n8), *d_m = st.in(trans_mean, n8), *d_sd = st.in(trans_sd, n8), *d_w = st.in(w.data(), n8);
    const double* d_init = st.in(init_ps, nb_init * n8);
    double *d_K[3] = {nullptr, nullptr, nullptr}, *d_P[2] = {st.work(p_bytes), st.work(p_bytes)};
    for (int k = 0; k < (power ? 3 : 1); ++k) d_K[k] = st.work(kk_bytes);
    mfs::GridUpdateArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n; a.T = T; a.B = B; a.ldp = ldp; a.lik_kind = lik_kind; a.n_lik = n_lik; a.lik_batched = lik_batched != 0;
    a.xs = d_xs; a.w = d_w; a.lik = st.in(lik, nb_lik * n_lik * 8); a.ys = st.in(ys, bt * 8);
    // (means, variances and first_nan are written whether the caller wants them or not)
    a.out_pdfs = st.out(out_pdfs, bt * n * 8);
    a.out_means = st.out(out_means, bt * 8, 0, mfs::Staging::kAlways);
    a.out_vars = st.out(out_vars, bt * 8, 0, mfs::Staging::kAlways);
    a.nell = st.out(out_nell, (size_t)B * 8);
    a.first_nan = st.out(out_first_nan, (size_t)B * 4, 0, mfs::Staging::kAlways);
    // characteristic functions (nz > 0): the table, one product buffer and two output blocks of cf_S steps each, at most
    // 64 MB a block unless one step is larger (gridfilter_kernel.hpp)
    const int m_pad = mfs::grid_pad(nz);
    const size_t cf_step_bytes = (size_t)B * nz * 16;
    int cf_S = 0;
    const double* d_zs = nullptr;
    double *d_E = nullptr, *d_C = nullptr, *d_cf[2] = {nullptr, nullptr};
    if (nz > 0) {
        const size_t fit = ((size_t)64 << 20) / cf_step_bytes;
        cf_S = fit < 1 ? 1 : fit > (size_t)T ? T : (int)fit;
        d_zs = st.in(zs, (size_t)nz * 8);
        d_E = st.work((size_t)2 * m_pad * n_pad * 8); d_C = st.work((size_t)2 * m_pad * ldp * 8);
        for (int j = 0; j < (cf_S < T ? 2 : 1); ++j) d_cf[j] = st.work(cf_step_bytes * cf_S);
    }
    if (st.err == hipSuccess) st.err = hipMemsetAsync(a.nell, 0, (size_t)B * 8, st.s);
    if (st.err == hipSuccess) st.err = hipMemsetAsync(a.first_nan, 0xff, (size_t)B * 4, st.s);   // -1
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
    // output block c (steps [c cf_S, ...)) to the host, on the copy stream once the block is filled: B rows of its steps'
    // pairs into out_cfs [B][T][nz][2]; one copy per replicate where the host pitch is beyond what a 2-D copy takes
    const bool cf_2d = nz > 0 && mfs::pitch_ok((size_t)T * nz * 16, device);
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
        if (st.err == hipSuccess) st.err = mfs::launch_grid_cf_store(nz, B, m_pad, ldp, cf_S, slot, d_C, a.first_nan, d_cf[j], st.s);
        if (slot == cf_S - 1 || t == T - 1) {
            if (st.err == hipSuccess) st.err = hipEventRecord(st.cx->ev[j], st.s);
            if (c >= 1) drain_cf(c - 1);      // one block behind: the copy of block c - 1 runs under the kernels of block c
            if (t == T - 1) drain_cf(c);
        }
    }
    st.download();
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

    mfs::Staging st(device, stream, true);
    const double *d_xs = st.in(xs, (size_t)n * 8), *d_w = st.in(w.data(), (size_t)n * 8), *d_zs = st.in(zs, (size_t)nz * 8);
    // the table; then a chunk's densities (uploaded row by row into the padded block), products and pairs (copied out per chunk)
    double *d_E = st.work((size_t)n_pad * 2 * m_pad * 8), *d_ps = st.work((size_t)R * n_pad * 8);
    double *d_C = st.work((size_t)R * 2 * m_pad * 8), *d_out = st.work((size_t)R * nz * 16);
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
