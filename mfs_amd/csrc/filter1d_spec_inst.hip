// filter1d_spec_inst.hip -- the specialised one-wave-per-SIMD builds of the fast 1-D kernel (SPEC template parameter of
// filter1d_fast_kernel: coefficient table in registers, live rows only, straight-line halves) for one quadrature order
// MFS_SPEC_N in 14..16, the only orders that have a one-wave build.  One translation unit per order so that `make -j`
// compiles them next to the order ranges of filter1d_inst.hip.  With -DMFS_SPEC_TRAITS the unit holds the fixed-traits builds
// of the order instead (StepTraits: mode, u-map and likelihood law compiled in), a second object per order.
#include "filter1d_fast.hpp"
#include "launch_util.hpp"
#include "registry.hpp"

#ifndef MFS_SPEC_N
#error "compile with -DMFS_SPEC_N=14..16"
#endif

namespace mfs {

template <int N, int G, int SPEC, class TR = StepTraits<>>
hipError_t launch_filter_spec(const Filter1dArgs& a, int grid, int lds_doubles, hipStream_t s) {
    if (hipError_t e = ensure_dynamic_lds<&filter1d_fast_kernel<N, G, 1, 1, false, SPEC, TR>>(); e != hipSuccess) return e;
    hipLaunchKernelGGL((filter1d_fast_kernel<N, G, 1, 1, false, SPEC, TR>), dim3(grid), dim3(64), (64 / G) * lds_doubles * 8, s,
                       a, lds_doubles);
    return hipGetLastError();
}

namespace {   // (one registrar per object file, each with its own constructor)
struct SpecRegistrar {
    SpecRegistrar() {
        constexpr int N = MFS_SPEC_N;
        static_assert(N >= 14 && N <= 16, "orders with a one-wave build");
        constexpr int gi = default_group(N), G = group_lanes(gi);   // the default lane count of the order, as for FastEntry::wide
#ifndef MFS_SPEC_TRAITS
        Filter1dFastLaunch* spec = g_fast[N][gi].spec;
        spec[spec_shape_index(-1)] = &launch_filter_spec<N, G, -1>;
        spec[spec_shape_index(2)] = &launch_filter_spec<N, G, 2>;
        spec[spec_shape_index(4)] = &launch_filter_spec<N, G, 4>;
        spec[spec_shape_index(6)] = &launch_filter_spec<N, G, 6>;
#else
        // the pairs a shipped model reaches: Benes-Bernoulli with TME-3 and TME-normal tables, OU-Gaussian (normal closure)
        using TanhBernoulli = StepTraits<MFS_MODE_CENTRAL, MFS_U_TANH, MFS_LIK_BERNOULLI_LOGISTIC>;
        using IdentityGaussian = StepTraits<MFS_MODE_CENTRAL, MFS_U_IDENTITY, MFS_LIK_GAUSSIAN>;
        constexpr int tb = MFS_TRAITS_CENTRAL_TANH_BERNOULLI - 1, ig = MFS_TRAITS_CENTRAL_IDENTITY_GAUSSIAN - 1;
        static_assert(traits_index(TanhBernoulli::mode, TanhBernoulli::umap, TanhBernoulli::lik) == tb + 1, "traits slot");
        static_assert(traits_index(IdentityGaussian::mode, IdentityGaussian::umap, IdentityGaussian::lik) == ig + 1, "traits slot");
        auto& st = g_fast[N][gi].spec_traits;
        st[spec_shape_index(6)][tb] = &launch_filter_spec<N, G, 6, TanhBernoulli>;
        st[spec_shape_index(-1)][tb] = &launch_filter_spec<N, G, -1, TanhBernoulli>;
        st[spec_shape_index(-1)][ig] = &launch_filter_spec<N, G, -1, IdentityGaussian>;
#endif
    }
};
SpecRegistrar spec_registrar_instance;
}  // namespace

}  // namespace mfs
