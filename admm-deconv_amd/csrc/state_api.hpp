// state_api.hpp -- host interface of the resumable solve's start / end kernels (state_kernels.hip).
//
// The whole per-pixel ADMM state is s_k = D x_k + u_{k-1} (z_k = prox(s_k), u_k = s_k - z_k), a plane set
// in the natural layout float[planes][2][N][M]: channel 0 = x[j][i] - x[j-1][i] (the difference along N), channel 1 =
// x[j][i] - x[j][i-1] (along M), periodic -- the layout of the 2-pass / runtime-length s buffers and trajectory slots.
// Every kernel here is elementwise plus periodic neighbours, any 2 <= M, N; sums are fp64 in a fixed order, no atomics.
// iso: the prox is BT with the batch's factor map f (M x N, from the norm step), z = f s; else ST at tau = prm[0].
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace admm {
namespace st {

constexpr int kResidSums = 5;   // |r|^2, |d|^2, |D x_K|^2, |z_K|^2, |rho D^T u_K|^2 per plane
// blocks per plane of the residual pass (partials: planes x resid_blocks x kResidSums doubles): about 4096 blocks in
// all, at least 2048 pixels and at most 64 blocks per plane -- a block ends in five LDS tree sums, so a large batch
// runs few blocks per plane and a single large plane many
inline int resid_blocks(size_t MN, size_t planes) {
    const size_t by_px = (MN + 2047) / 2048, by_planes = (4096 + planes - 1) / planes;
    size_t nb = by_px < by_planes ? by_px : by_planes;
    if (nb > 64) nb = 64;
    return nb < 1 ? 1 : (int)nb;
}

// start: v_0 = rho D^T (z_0 - u_0) of s_0, one M x N plane per plane (fmap NULL: ST)
hipError_t launch_v0(const float* s0, const float* fmap, float* v0, int M, int N, size_t planes, const float* prm,
                     hipStream_t s);
// the plane groups' partial sums of s^2 over both channels (iso_r_kernel's input: group g's map at part + g M N)
hipError_t launch_sq(const float* s, float* part, size_t MN, size_t planes, int G, int ngroups, hipStream_t s_);
// end: s_K = D x_K + u_{K-1}, u_{K-1} from s_prev (NULL: zero state) and, isotropic, its factor map
hipError_t launch_end(const float* x, const float* s_prev, const float* fmap_prev, bool iso, float* s_out, int M, int N,
                      size_t planes, const float* prm, hipStream_t s);
// residual norms per plane: out[plane] = {|r|, |d|, max(|D x_K|, |z_K|), rho |D^T u_K|}; partial: the blocks' sums
hipError_t launch_resid(const float* sK, const float* s_prev, const float* fK, const float* f_prev, bool iso,
                        double* partial, float* out, int M, int N, size_t planes, const float* prm, hipStream_t s);

}  // namespace st
}  // namespace admm
