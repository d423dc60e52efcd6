// filter1d_partner_inst.hip -- the partner-wave variant (filter1d_partner.hpp) of the fixed-traits specialised one-wave builds
// for one quadrature order MFS_SPEC_N in 14..15.  A translation unit of its own: the one-wave builds' objects do not change
// with it.
#include "filter1d_partner.hpp"
#include "launch_util.hpp"
#include "registry.hpp"

#ifndef MFS_SPEC_N
#error "compile with -DMFS_SPEC_N=14..15"
#endif

namespace mfs {

template <int N, int G, int SPEC, class TR>
hipError_t launch_filter_partner(const Filter1dArgs& a, int grid, int lds_doubles, hipStream_t s) {
    const int lds_bytes = partner_lds_bytes(lds_doubles, PartnerTile<N, G>::kDoubles);
    if (lds_bytes > kPartnerLdsMax) return hipErrorInvalidValue;
    if (hipError_t e = ensure_dynamic_lds<&filter1d_partner_kernel<N, G, SPEC, TR>>(kPartnerLdsMax); e != hipSuccess) return e;
    hipLaunchKernelGGL((filter1d_partner_kernel<N, G, SPEC, TR>), dim3(grid), dim3(kPartnerThreads), lds_bytes, s, a, lds_doubles);
    return hipGetLastError();
}

// this unit's copy of the placement counters (filter1d_partner.hpp): [0] workgroups checked, [1] mismatches
static hipError_t read_partner_placement(unsigned long long* counts) {
    return hipMemcpyFromSymbol(counts, HIP_SYMBOL(g_partner_placement), 2 * sizeof(*counts));
}

namespace {
struct PartnerRegistrar {
    PartnerRegistrar() {
        constexpr int N = MFS_SPEC_N;
        static_assert(N >= 14 && N <= 15, "orders with 16 lanes per filter and a one-wave build");
        constexpr int gi = default_group(N), G = group_lanes(gi);
        static_assert(G == 16, "lanes per filter");
        static_assert(kPartnerFilters == kPartnerMainWaves * (64 / G), "filters per workgroup");
        using TanhBernoulli = StepTraits<MFS_MODE_CENTRAL, MFS_U_TANH, MFS_LIK_BERNOULLI_LOGISTIC>;
        using IdentityGaussian = StepTraits<MFS_MODE_CENTRAL, MFS_U_IDENTITY, MFS_LIK_GAUSSIAN>;
        constexpr int tb = MFS_TRAITS_CENTRAL_TANH_BERNOULLI - 1, ig = MFS_TRAITS_CENTRAL_IDENTITY_GAUSSIAN - 1;
        FastEntry& fe = g_fast[N][gi];
        fe.partner[spec_shape_index(6)][tb] = &launch_filter_partner<N, G, 6, TanhBernoulli>;
        fe.partner[spec_shape_index(-1)][tb] = &launch_filter_partner<N, G, -1, TanhBernoulli>;
        fe.partner[spec_shape_index(-1)][ig] = &launch_filter_partner<N, G, -1, IdentityGaussian>;
        fe.partner_doubles = PartnerTile<N, G>::kDoubles;
        fe.partner_placement = &read_partner_placement;
    }
};
PartnerRegistrar partner_registrar_instance;
}  // namespace

}  // namespace mfs
