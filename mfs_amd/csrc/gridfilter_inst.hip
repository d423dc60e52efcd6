// gridfilter_inst.hip -- the brute-force grid filter's kernels (gridfilter_kernel.hpp) and their launchers (registry.hpp).
#include "gridfilter_kernel.hpp"

namespace mfs {

hipError_t launch_grid_build_k(int n, int n_pad, const double* d_xs, const double* d_mean, const double* d_sd,
                               const double* d_w, double* d_K, hipStream_t s) {
    hipLaunchKernelGGL(grid_build_k, dim3(n_pad / 64, n_pad), dim3(64), 0, s, n, n_pad, d_xs, d_mean, d_sd, d_w, d_K);
    return hipGetLastError();
}

hipError_t launch_grid_init_p(int n, int n_pad, int B, int ldp, const double* d_init, int init_batched, double* d_P,
                              hipStream_t s) {
    hipLaunchKernelGGL(grid_init_p, dim3(ldp / 64, n_pad), dim3(64), 0, s, n, B, ldp, d_init, init_batched, d_P);
    return hipGetLastError();
}

hipError_t launch_grid_gemm(int M, int N, int Kd, const double* d_A, const double* d_B, double* d_C, hipStream_t s) {
    if (M <= 0 || N <= 0 || Kd <= 0 || M % kGridTile || N % kGridTile || Kd % kGridBK || d_C == d_A || d_C == d_B)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(grid_gemm, dim3(N / kGridTile, M / kGridTile), dim3(256), 0, s, d_A, (size_t)Kd, d_B, (size_t)N, d_C,
                       (size_t)N, Kd);
    return hipGetLastError();
}

hipError_t launch_grid_update(const GridUpdateArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(grid_update, dim3((a.B + kGridCols - 1) / kGridCols), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_grid_cf_table(int n, int nz, int n_pad, int m_pad, int transposed, const double* d_xs, const double* d_w,
                                const double* d_zs, double* d_E, hipStream_t s) {
    const dim3 grid = transposed ? dim3(m_pad / 64, n_pad) : dim3(n_pad / 64, m_pad);
    hipLaunchKernelGGL(grid_cf_table, grid, dim3(64), 0, s, n, nz, n_pad, m_pad, transposed, d_xs, d_w, d_zs, d_E);
    return hipGetLastError();
}

hipError_t launch_grid_cf_store(int nz, int B, int m_pad, int ldp, int S, int slot, const double* d_C, const int32_t* d_first_nan,
                                double* d_out, hipStream_t s) {
    hipLaunchKernelGGL(grid_cf_store, dim3(ldp / kGridCfTile, m_pad / kGridCfTile), dim3(256), 0, s, nz, B, m_pad, ldp, S, slot,
                       d_C, d_first_nan, reinterpret_cast<double2*>(d_out));
    return hipGetLastError();
}

hipError_t launch_grid_cf_store_rows(int rows, int nz, int m_pad, const double* d_C, double* d_out, hipStream_t s) {
    hipLaunchKernelGGL(grid_cf_store_rows, dim3(m_pad / 64, rows), dim3(64), 0, s, nz, m_pad, d_C,
                       reinterpret_cast<double2*>(d_out));
    return hipGetLastError();
}

}  // namespace mfs
