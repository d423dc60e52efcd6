// diagnostic: the library sources compiled with phase stamps + an accessor (never part of libmfs_hip.so)
#define MFS_1D_STAMPS
#define MFS_NLO 15
#define MFS_NHI 15
#define MFS_SPEC_N 15
#include "../../mfs_amd/csrc/filter1d_inst.hip"
#include "../../mfs_amd/csrc/filter1d_spec_inst.hip"
extern "C" int mfs_debug_stamps(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(mfs::g_1d_stamps), 32 * sizeof(unsigned long long));
}
extern "C" int mfs_debug_stamps_reset(void) {
    static const unsigned long long zero[32] = {0};
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(mfs::g_1d_stamps), zero, sizeof(zero));
}
