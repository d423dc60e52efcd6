// filternd3_inst.hip -- instantiates the d = 3 N-D kernels for N = 2..4 and both transition families (TK = 0 operator tables,
// TK = 1 Normal closure), without and with joint likelihood factors, and registers their launchers.
#include "filternd3_kernel.hpp"
#include "launch_util.hpp"
#include "registry.hpp"

namespace mfs {

Nd3Entry g_nd3_table[MFS_ND3_MAX_N + 1];

template <int N, int TK>
hipError_t launch_nd3(const FilterNd3Args& a, int grid, hipStream_t s) {
    constexpr int lds = Nd3Tile<N>::kDoubles * 8;
    if (hipError_t e = ensure_dynamic_lds<&filternd3_kernel<N, TK>>(); e != hipSuccess) return e;
    hipLaunchKernelGGL((filternd3_kernel<N, TK>), dim3(grid), dim3(256), lds, s, a);
    return hipGetLastError();
}

template <int N, int TK>
hipError_t launch_nd3_joint(const FilterNd3Args& a, const FilterNd3Joint& jt, int grid, hipStream_t s) {
    constexpr int lds = Nd3Tile<N>::kDoubles * 8;
    if (hipError_t e = ensure_dynamic_lds<&filternd3_joint_kernel<N, TK>>(); e != hipSuccess) return e;
    hipLaunchKernelGGL((filternd3_joint_kernel<N, TK>), dim3(grid), dim3(256), lds, s, a, jt);
    return hipGetLastError();
}

template <int N>
void reg_nd3() {
    g_nd3_table[N] = Nd3Entry{&launch_nd3<N, 0>, &launch_nd3<N, 1>, Nd3Tile<N>::S, Nd3Tile<N>::Z, Nd3Tile<N>::kDoubles * 8,
                              &launch_nd3_joint<N, 0>, &launch_nd3_joint<N, 1>};
    if constexpr (N < MFS_ND3_MAX_N) reg_nd3<N + 1>();
}

struct Nd3Registrar { Nd3Registrar() { reg_nd3<MFS_ND3_MIN_N>(); } };
static Nd3Registrar nd3_registrar_instance;

}  // namespace mfs
