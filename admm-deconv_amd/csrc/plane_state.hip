// plane_state.hip -- the fused per-plane kernel's STATE instantiations (plane256_kernel<PSF, 0, 3>: the resumable solve
// at 256 x 256 anisotropic, admm_tvd_forward_state_dev_f32), the kernels that carry the state between the natural layout
// of the ABI and the kernel's lane-native s, and their host launchers -- in a translation unit of their own, as
// plane_grouped_rec.hip and for its reason: the code objects of plane_launch.hip and plane_grouped_rec.hip stay byte for
// byte what they are.
//
// plane_kernel.hip defines two small non-template kernels and a device variable; this unit's copies get names of
// their own, so that the library links (they are not used here).
#define tables_kernel tables_kernel_state
#define dx_lane_kernel dx_lane_kernel_state
#define g_plane_ts g_plane_ts_state
#include "plane_api.hpp"
#include "plane_kernel.hip"

namespace admm {
namespace plane {

// Thread -> pixel pair of the two kernels below: a block is 4 lines x half a line, a wave 64 consecutive pixel pairs of
// one line.  The natural-layout accesses (most of the bytes) are then 512 contiguous bytes per wave, and the four lines
// of a block fill whole 128-byte lines of the lane-native array (entries t = 2r .. 2r + 7 of a register n).
struct PairOf {
    int r, p, idx;   // line, first pixel of the pair, lane-native entry [n][t]
};
__device__ __forceinline__ PairOf pair_of() {
    const int r = (blockIdx.x >> 1) * 4 + (threadIdx.x >> 6);
    const int p2 = (blockIdx.x & 1) * 64 + (threadIdx.x & 63);
    return {r, 2 * p2, (p2 >> 1) * kPT + 2 * r + (p2 & 1)};
}

// s_0 (natural layout, planes x 2 x 256 x 256) -> the kernel's lane-native s: entry [n][t] = (s0[p], s0[p+1], s1[p],
// s1[p+1]) of pixel pair p = 4n + 2h of line r, t = 2r + h (dx_lane_kernel's layout).  grid (128, planes) x 256.
__global__ __launch_bounds__(256) void state_import_kernel(const float* __restrict__ s_in, float4* __restrict__ sln) {
    const PairOf q = pair_of();
    const int r = q.r, p = q.p, idx = q.idx;
    const float* sp = s_in + (size_t)blockIdx.y * 2 * 65536 + r * 256 + p;
    const float2 a = *reinterpret_cast<const float2*>(sp);
    const float2 b = *reinterpret_cast<const float2*>(sp + 65536);
    sln[(size_t)blockIdx.y * 64 * kPT + idx] = make_float4(a.x, a.y, b.x, b.y);
}

// s_K = D x_K + clip(s_{K-1}) in the natural layout, from the output and the kernel's lane-native s_{K-1} (sln NULL: K =
// 1 from the zero state, u_0 = 0); s_prev, when given, receives s_{K-1} in the natural layout as well (the residual pass
// reads neighbours of both).  grid (128, planes) x 256.
__global__ __launch_bounds__(256) void state_end_lane_kernel(const float* __restrict__ x, const float4* __restrict__ sln,
                                                             float* __restrict__ s_out, float* __restrict__ s_prev,
                                                             const float* __restrict__ prm) {
    const float tau = prm[0];
    const PairOf q = pair_of();
    const int r = q.r, p = q.p, idx = q.idx;
    const float* xp = x + (size_t)blockIdx.y * 65536;
    const float2 c = *reinterpret_cast<const float2*>(xp + r * 256 + p);
    const float2 u = *reinterpret_cast<const float2*>(xp + ((r + 255) & 255) * 256 + p);
    const float l = xp[r * 256 + ((p + 255) & 255)];
    float4 so = make_float4(0.f, 0.f, 0.f, 0.f);
    if (sln) so = sln[(size_t)blockIdx.y * 64 * kPT + idx];
    const float4 s = make_float4(c.x - u.x + clip_tau(so.x, tau), c.y - u.y + clip_tau(so.y, tau),
                                 c.x - l + clip_tau(so.z, tau), c.y - c.x + clip_tau(so.w, tau));
    const size_t o = (size_t)blockIdx.y * 2 * 65536 + r * 256 + p;
    *reinterpret_cast<float2*>(s_out + o) = make_float2(s.x, s.y);
    *reinterpret_cast<float2*>(s_out + o + 65536) = make_float2(s.z, s.w);
    if (s_prev) {
        *reinterpret_cast<float2*>(s_prev + o) = make_float2(so.x, so.y);
        *reinterpret_cast<float2*>(s_prev + o + 65536) = make_float2(so.z, so.w);
    }
}

template <bool PSF>
static void launch_one_state(const float* y, float* x_out, const void* tables, float2* hln, float4* sln, const float* prm,
                             int K, size_t planes, hipStream_t s, const float* v0) {
    float* Cf = static_cast<float*>(const_cast<void*>(tables));   // the lane-native table block (plane_launch.hip carve)
    float* C0b = Cf + kTab;
    float2* Gf = reinterpret_cast<float2*>(C0b + 256);
    float2* G0b = Gf + kTab;
    (void)hipFuncSetAttribute((const void*)plane256_kernel<PSF, 0, 3>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)kLdsBytes);
    hipLaunchKernelGGL((plane256_kernel<PSF, 0, 3>), dim3((unsigned)planes), dim3(kPT), kLdsBytes, s, y, x_out, Cf, C0b, Gf,
                       G0b, hln, sln, prm, K, nullptr, nullptr, planes * 64 * kPT, Branches{1, 1, 1, 0u, 0u},
                       reinterpret_cast<unsigned*>(const_cast<float*>(v0)), planes * 16 * kPT);
}

hipError_t launch_plane_state(const float* y, float* x_out, const void* tables, bool psf, float2* hln, float4* sln,
                              const float* prm, int K, size_t planes, hipStream_t s, const float* state_in,
                              const float* v0) {
    if ((state_in != nullptr) != (v0 != nullptr)) return hipErrorInvalidValue;
    if (state_in) {
        hipLaunchKernelGGL(state_import_kernel, dim3(64 * kPT / 256, (unsigned)planes), dim3(256), 0, s, state_in, sln);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (psf) launch_one_state<true>(y, x_out, tables, hln, sln, prm, K, planes, s, v0);
    else launch_one_state<false>(y, x_out, tables, hln, sln, prm, K, planes, s, v0);
    return hipGetLastError();
}

hipError_t launch_state_end_lane(const float* x, const float4* sln, float* s_out, float* s_prev, const float* prm,
                                 size_t planes, hipStream_t s) {
    hipLaunchKernelGGL(state_end_lane_kernel, dim3(64 * kPT / 256, (unsigned)planes), dim3(256), 0, s, x, sln, s_out, s_prev,
                       prm);
    return hipGetLastError();
}

}  // namespace plane
}  // namespace admm
