// plane_grouped_rec.hip -- the fused per-plane kernel's grouped RECORDING instantiations (plane256_kernel<PSF, 0, 1,
// GRP>: a grouped solve that writes s_k lane-native into its trajectory slots, for the grouped adjoint) and their host
// launcher, in a translation unit of their own.
//
// Why not plane_launch.hip: the c2 kernel's speed depends on where it lands in its code object (DESIGN.md s5 "Grouped
// solve": +-1 % from placement).  Two more instantiations at the END of plane_launch.hip left every existing
// instruction stream identical and still moved .text by 4352 bytes (more kernel descriptors, symbols and metadata
// ahead of it): c2 ran 1.5-2 % slower in ten alternating runs, and only the object of that translation unit mattered
// (profiles/grouped_adjoint_bench.json).  Here the existing code object stays byte for byte what it was.
//
// plane_kernel.hip defines two small non-template kernels and a device variable; this unit's copies get names of
// their own, so that the library links (they are not used here).
#define tables_kernel tables_kernel_grec
#define dx_lane_kernel dx_lane_kernel_grec
#define g_plane_ts g_plane_ts_grec
#include "plane_api.hpp"
#include "plane_kernel.hip"

namespace admm {
namespace plane {

template <bool PSF>
static void launch_one_grouped_rec(const float* y, float* x_out, const void* tables, float2* hln, float4* sln,
                                   const float* prm, int K, size_t planes, hipStream_t s, const Branches& br,
                                   float4* traj) {
    // the lane-native table block of group 0 (plane_launch.hip carve); the kernel offsets it by the plane's group
    float* Cf = static_cast<float*>(const_cast<void*>(tables));
    float* C0b = Cf + kTab;
    float2* Gf = reinterpret_cast<float2*>(C0b + 256);
    float2* G0b = Gf + kTab;
    (void)hipFuncSetAttribute((const void*)plane256_kernel<PSF, 0, 1, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)kLdsBytes);
    hipLaunchKernelGGL((plane256_kernel<PSF, 0, 1, true>), dim3((unsigned)planes), dim3(kPT), kLdsBytes, s, y, x_out, Cf,
                       C0b, Gf, G0b, hln, sln, prm, K, nullptr, traj, planes * 64 * kPT, br, nullptr, planes * 16 * kPT);
}

hipError_t launch_plane_grouped_rec(const float* y, float* x_out, const void* tables, bool psf, float2* hln, float4* sln,
                                    const float* prm, int K, size_t planes, hipStream_t s, float4* traj,
                                    const Branches& br) {
    if (br.nbr != 0 || !traj) return hipErrorInvalidValue;
    if (psf) launch_one_grouped_rec<true>(y, x_out, tables, hln, sln, prm, K, planes, s, br, traj);
    else launch_one_grouped_rec<false>(y, x_out, tables, hln, sln, prm, K, planes, s, br, traj);
    return hipGetLastError();
}

}  // namespace plane
}  // namespace admm
