// particle_nd_inst.hip -- the d = 2 bootstrap particle filter's kernels (particle_nd_kernel.hpp) and their launchers
// (registry.hpp).  The `offsets` kernel of a step is the one in particle_inst.hip, which serves every state dimension.
#include "particle_nd_kernel.hpp"

namespace mfs {

static dim3 pfnd_grid(const PfNdArgs& a) { return dim3(a.nblk, a.B); }

hipError_t launch_pfnd_init(const PfNdArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pfnd_init, pfnd_grid(a), dim3(kPfThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_pfnd_propagate(const PfNdArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pfnd_propagate, pfnd_grid(a), dim3(kPfThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_pfnd_resample(const PfNdArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pfnd_resample, pfnd_grid(a), dim3(kPfThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_pfnd_cov(const PfNdArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pfnd_cov, dim3(a.nseg, a.B), dim3(kPfThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_pfnd_finalize(const PfNdArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pfnd_finalize, dim3(a.B), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace mfs
