// particle_inst.hip -- the bootstrap particle filter's kernels (particle_kernel.hpp) and their launchers (registry.hpp).
#include "particle_kernel.hpp"

namespace mfs {

static dim3 pf_grid(const PfArgs& a) { return dim3(a.nblk, a.B); }

hipError_t launch_pf_init(const PfArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pf_init, pf_grid(a), dim3(kPfThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_pf_propagate(const PfArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pf_propagate, pf_grid(a), dim3(kPfThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_pf_offsets(const PfOffsetsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pf_offsets, dim3((a.B + 63) / 64), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_pf_resample(const PfArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pf_resample, pf_grid(a), dim3(kPfThreads), 0, s, a);
    return hipGetLastError();
}

// frequencies per thread: the smallest of 1, 2, 4, 8 with which one block covers the grid, else 8 and several chunks
hipError_t launch_pf_cf(const PfArgs& a, hipStream_t s) {
    const int F = (a.nz <= kPfThreads) ? 1 : (a.nz <= 2 * kPfThreads) ? 2 : (a.nz <= 4 * kPfThreads) ? 4 : kPfMaxF;
    const int chunks = (a.nz > 0) ? (a.nz + kPfThreads * F - 1) / (kPfThreads * F) : 1;
    const dim3 grid(a.nseg, a.B, chunks), block(kPfThreads);
    if (F == 1) hipLaunchKernelGGL(pf_cf<1>, grid, block, 0, s, a);
    else if (F == 2) hipLaunchKernelGGL(pf_cf<2>, grid, block, 0, s, a);
    else if (F == 4) hipLaunchKernelGGL(pf_cf<4>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(pf_cf<kPfMaxF>, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_pf_finalize(const PfArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pf_finalize, dim3((2 * a.nz + 2 + kPfThreads - 1) / kPfThreads, a.B), dim3(kPfThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_pf_draws(uint64_t seed, int t, int tag, int draw, int count, double* d_uniform, double* d_normal,
                           hipStream_t s) {
    hipLaunchKernelGGL(pf_draws, dim3((count + kPfThreads - 1) / kPfThreads), dim3(kPfThreads), 0, s, seed, t, tag, draw, count,
                       d_uniform, d_normal);
    return hipGetLastError();
}

}  // namespace mfs
