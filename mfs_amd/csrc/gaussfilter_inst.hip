// gaussfilter_inst.hip -- the Gaussian filters' kernels (gaussfilter_kernel.hpp) and their launcher (registry.hpp).
#include "gaussfilter_kernel.hpp"

namespace mfs {

// the LDS layout of gf_filter_1d / gf_filter_2d: points, weights, model table(s), likelihood parameters
int gf_lds_bytes(const GfArgs& a) {
    const int n = (a.method == MFS_GF_EKF) ? 0 : a.n_points, G = kGfThreads / a.lanes;
    int doubles;
    if (a.d == 1)
        doubles = 2 * n + (a.coef_batched ? G : 1) * 2 * (a.degree + 1) + (a.lik_batched ? G : 1) * a.n_lik;
    else
        doubles = 3 * n + 5 * a.extent * a.extent + (a.lik_batched ? G : 1) * MFS_MAX_LIK;
    return doubles * (int)sizeof(double);
}

template <int L, bool EKF>
static hipError_t gf_launch(const GfArgs& a, hipStream_t s) {
    const dim3 grid((a.B + kGfThreads / L - 1) / (kGfThreads / L)), block(kGfThreads);
    if (a.d == 1) hipLaunchKernelGGL((gf_filter_1d<L, EKF>), grid, block, gf_lds_bytes(a), s, a);
    else hipLaunchKernelGGL((gf_filter_2d<L, EKF>), grid, block, gf_lds_bytes(a), s, a);
    return hipGetLastError();
}

hipError_t launch_gauss_filter(const GfArgs& a, hipStream_t s) {
    if (a.method == MFS_GF_EKF) return gf_launch<1, true>(a, s);
    switch (a.lanes) {
        case 1: return gf_launch<1, false>(a, s);
        case 2: return gf_launch<2, false>(a, s);
        case 4: return gf_launch<4, false>(a, s);
        case 8: return gf_launch<8, false>(a, s);
        case 16: return gf_launch<16, false>(a, s);
        case 32: return gf_launch<32, false>(a, s);
        case 64: return gf_launch<64, false>(a, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace mfs
