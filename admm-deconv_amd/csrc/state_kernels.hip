// state_kernels.hip -- start and end kernels of the resumable solve (admm_tvd_forward_state_dev_f32), in a translation
// unit of their own: the code objects of the iteration kernels stay what they are.  Interface and layout: state_api.hpp.
//   start   v_0 = rho D^T (z_0 - u_0) from the caller's s_0 (sq_kernel + the library's norm step first when isotropic);
//           the path's line transform then turns v_0 into the first line spectrum, in place of the cold call's zeros
//   end     s_K = D x_K + u_{K-1} from the output and s_{K-1}; the four norms of the ADMM stopping rule per plane
// The prox expressions are the iteration kernels' own (admm_kernels.hip line_body / iso_a / iso_b): u = clip(s, tau)
// and w = z - u = phi(s) for ST, u = s - f s and w = f s - (s - f s) for BT.
#include "state_api.hpp"

namespace admm {
namespace st {

namespace {

constexpr int kT = 256;

__device__ __forceinline__ float clipf(float s, float tau) { return fminf(fmaxf(s, -tau), tau); }
__device__ __forceinline__ float prox_w(float s, float tau) { return fabsf(s) > tau ? s - copysignf(2.0f * tau, s) : -s; }
// u = s - prox(s)
__device__ __forceinline__ float dual_of(float s, float f, float tau, bool iso) { return iso ? s - f * s : clipf(s, tau); }
// w = prox(s) - u
__device__ __forceinline__ float w_of(float s, float f, float tau, bool iso) {
    return iso ? f * s - (s - f * s) : prox_w(s, tau);
}

// grid (blocks, planes)
__global__ __launch_bounds__(kT) void v0_kernel(const float* __restrict__ s0, const float* __restrict__ fmap,
                                                float* __restrict__ v0, int M, int N, const float* __restrict__ prm) {
    const float tau = prm[0], rho = prm[1];
    const bool iso = fmap != nullptr;
    const size_t MN = (size_t)M * N;
    const float* sp = s0 + (size_t)blockIdx.y * 2 * MN;
    float* vp = v0 + (size_t)blockIdx.y * MN;
    for (size_t q = (size_t)blockIdx.x * kT + threadIdx.x; q < MN; q += (size_t)gridDim.x * kT) {
        const int j = (int)(q / M), i = (int)(q - (size_t)j * M);
        const size_t qd = (size_t)(j + 1 == N ? 0 : j + 1) * M + i;   // next line
        const size_t qr = (size_t)j * M + (i + 1 == M ? 0 : i + 1);   // next pixel
        const float f = iso ? fmap[q] : 0.0f, fd = iso ? fmap[qd] : 0.0f, fr = iso ? fmap[qr] : 0.0f;
        const float a = w_of(sp[q], f, tau, iso), b = w_of(sp[qd], fd, tau, iso);
        const float c = w_of(sp[MN + q], f, tau, iso), cn = w_of(sp[MN + qr], fr, tau, iso);
        vp[q] = rho * ((a - b) + (c - cn));
    }
}

// grid (blocks, plane groups): group g sums planes g G .. in plane order
__global__ __launch_bounds__(kT) void sq_kernel(const float* __restrict__ s, float* __restrict__ part, size_t MN,
                                                int planes, int G) {
    const int g = blockIdx.y;
    const int p0 = g * G, p1 = min(planes, p0 + G);
    for (size_t q = (size_t)blockIdx.x * kT + threadIdx.x; q < MN; q += (size_t)gridDim.x * kT) {
        float acc = 0.0f;
        for (int p = p0; p < p1; ++p) {
            const float a = s[(size_t)p * 2 * MN + q], b = s[(size_t)p * 2 * MN + MN + q];
            acc += a * a + b * b;
        }
        part[(size_t)g * MN + q] = acc;
    }
}

// grid (blocks, planes)
__global__ __launch_bounds__(kT) void end_kernel(const float* __restrict__ x, const float* __restrict__ s_prev,
                                                 const float* __restrict__ fmap_prev, int iso, float* __restrict__ s_out,
                                                 int M, int N, const float* __restrict__ prm) {
    const float tau = prm[0];
    const size_t MN = (size_t)M * N;
    const float* xp = x + (size_t)blockIdx.y * MN;
    const float* sp = s_prev ? s_prev + (size_t)blockIdx.y * 2 * MN : nullptr;
    float* so = s_out + (size_t)blockIdx.y * 2 * MN;
    for (size_t q = (size_t)blockIdx.x * kT + threadIdx.x; q < MN; q += (size_t)gridDim.x * kT) {
        const int j = (int)(q / M), i = (int)(q - (size_t)j * M);
        const float xc = xp[q];
        const float xu = xp[(size_t)(j == 0 ? N - 1 : j - 1) * M + i];
        const float xl = xp[(size_t)j * M + (i == 0 ? M - 1 : i - 1)];
        float u0 = 0.0f, u1 = 0.0f;
        if (sp) {
            const float f = iso ? fmap_prev[q] : 0.0f;
            u0 = dual_of(sp[q], f, tau, iso != 0);
            u1 = dual_of(sp[MN + q], f, tau, iso != 0);
        }
        so[q] = (xc - xu) + u0;
        so[MN + q] = (xc - xl) + u1;
    }
}

struct ZU {
    double z, u;
};
__device__ __forceinline__ ZU zu_of(const float* __restrict__ s, const float* __restrict__ f, size_t q, float tau,
                                    bool iso) {
    if (!s) return {0.0, 0.0};
    const float v = s[q];
    const float u = dual_of(v, iso ? f[q] : 0.0f, tau, iso);
    return {(double)v - (double)u, (double)u};
}

// grid (resid_blocks, planes): the block's five sums, lanes combined by a fixed LDS tree
__global__ __launch_bounds__(kT) void resid_kernel(const float* __restrict__ sK, const float* __restrict__ s_prev,
                                                   const float* __restrict__ fK, const float* __restrict__ f_prev, int iso_,
                                                   double* __restrict__ partial, int M, int N,
                                                   const float* __restrict__ prm) {
    const float tau = prm[0];
    const double rho = (double)prm[1];
    const bool iso = iso_ != 0;
    const size_t MN = (size_t)M * N;
    const float* k0 = sK + (size_t)blockIdx.y * 2 * MN;
    const float* k1 = k0 + MN;
    const float* p0 = s_prev ? s_prev + (size_t)blockIdx.y * 2 * MN : nullptr;
    const float* p1 = p0 ? p0 + MN : nullptr;
    double acc[kResidSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (size_t q = (size_t)blockIdx.x * kT + threadIdx.x; q < MN; q += (size_t)gridDim.x * kT) {
        const int j = (int)(q / M), i = (int)(q - (size_t)j * M);
        const size_t qd = (size_t)(j + 1 == N ? 0 : j + 1) * M + i;
        const size_t qr = (size_t)j * M + (i + 1 == M ? 0 : i + 1);
        const ZU a0 = zu_of(k0, fK, q, tau, iso), a1 = zu_of(k1, fK, q, tau, iso);          // z_K, u_K here
        const ZU b0 = zu_of(p0, f_prev, q, tau, iso), b1 = zu_of(p1, f_prev, q, tau, iso);  // z_{K-1}, u_{K-1}
        const ZU ad = zu_of(k0, fK, qd, tau, iso), bd = zu_of(p0, f_prev, qd, tau, iso);    // channel 0, next line
        const ZU ar = zu_of(k1, fK, qr, tau, iso), br = zu_of(p1, f_prev, qr, tau, iso);    // channel 1, next pixel
        // D x_K = s_K - u_{K-1};  r = D x_K - z_K
        const double dx0 = (double)k0[q] - b0.u, dx1 = (double)k1[q] - b1.u;
        const double r0 = dx0 - a0.z, r1 = dx1 - a1.z;
        acc[0] += r0 * r0 + r1 * r1;
        // d = rho D^T (z_K - z_{K-1})
        const double d = rho * (((a0.z - b0.z) - (ad.z - bd.z)) + ((a1.z - b1.z) - (ar.z - br.z)));
        acc[1] += d * d;
        acc[2] += dx0 * dx0 + dx1 * dx1;
        acc[3] += a0.z * a0.z + a1.z * a1.z;
        const double du = rho * ((a0.u - ad.u) + (a1.u - ar.u));
        acc[4] += du * du;
    }
    __shared__ double red[kT];
#pragma unroll
    for (int k = 0; k < kResidSums; ++k) {
        red[threadIdx.x] = acc[k];
        __syncthreads();
        for (int w = kT / 2; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) partial[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kResidSums + k] = red[0];
        __syncthreads();
    }
}

// one thread per plane: the blocks' sums in block order
__global__ __launch_bounds__(kT) void resid_fin_kernel(const double* __restrict__ partial, int nblk, size_t planes,
                                                       float* __restrict__ out) {
    const size_t p = (size_t)blockIdx.x * kT + threadIdx.x;
    if (p >= planes) return;
    double a[kResidSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < nblk; ++b)
#pragma unroll
        for (int k = 0; k < kResidSums; ++k) a[k] += partial[(p * nblk + b) * kResidSums + k];
    out[p * 4 + 0] = (float)sqrt(a[0]);
    out[p * 4 + 1] = (float)sqrt(a[1]);
    out[p * 4 + 2] = (float)sqrt(fmax(a[2], a[3]));
    out[p * 4 + 3] = (float)sqrt(a[4]);
}

unsigned pixel_blocks(size_t MN) {
    const size_t nb = (MN + kT - 1) / kT;
    return nb > 256 ? 256u : (unsigned)nb;
}

}  // namespace

hipError_t launch_v0(const float* s0, const float* fmap, float* v0, int M, int N, size_t planes, const float* prm,
                     hipStream_t s) {
    hipLaunchKernelGGL(v0_kernel, dim3(pixel_blocks((size_t)M * N), (unsigned)planes), dim3(kT), 0, s, s0, fmap, v0, M, N,
                       prm);
    return hipGetLastError();
}

hipError_t launch_sq(const float* s, float* part, size_t MN, size_t planes, int G, int ngroups, hipStream_t s_) {
    hipLaunchKernelGGL(sq_kernel, dim3(pixel_blocks(MN), (unsigned)ngroups), dim3(kT), 0, s_, s, part, MN, (int)planes, G);
    return hipGetLastError();
}

hipError_t launch_end(const float* x, const float* s_prev, const float* fmap_prev, bool iso, float* s_out, int M, int N,
                      size_t planes, const float* prm, hipStream_t s) {
    hipLaunchKernelGGL(end_kernel, dim3(pixel_blocks((size_t)M * N), (unsigned)planes), dim3(kT), 0, s, x, s_prev,
                       fmap_prev, iso ? 1 : 0, s_out, M, N, prm);
    return hipGetLastError();
}

hipError_t launch_resid(const float* sK, const float* s_prev, const float* fK, const float* f_prev, bool iso,
                        double* partial, float* out, int M, int N, size_t planes, const float* prm, hipStream_t s) {
    const int nb = resid_blocks((size_t)M * N, planes);
    hipLaunchKernelGGL(resid_kernel, dim3((unsigned)nb, (unsigned)planes), dim3(kT), 0, s, sK, s_prev, fK, f_prev,
                       iso ? 1 : 0, partial, M, N, prm);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(resid_fin_kernel, dim3((unsigned)((planes + kT - 1) / kT)), dim3(kT), 0, s, partial, nb, planes, out);
    return hipGetLastError();
}

}  // namespace st
}  // namespace admm
