// plane_kernel.hip -- the whole K-iteration anisotropic ADMM solve of one 256 x 256 plane in ONE
// workgroup (reference: tvd_fft_cpu/tvd_fft_gpu, /root/reference/src/ops/ops.jl:46-93 / :132-176).
//
// Why: the 2-pass path (column kernel + line kernel per iteration, admm_kernels.hip) moves the line
// spectrum through HBM twice per iteration (36 B/px/iter).  Here the spectrum never leaves the CU:
// 512 threads = 256 lines x a lane pair (line_pair.hpp) hold it in registers; the dim-2 transforms go
// through a 132 KiB LDS column buffer in two halves of 64 spectral columns.  The only HBM traffic per
// iteration is the ADMM state s = Dx + u (read + write, 8 B/px each) and H^T y (4 B/px): 20 B/px/iter.
// Both are kept in a LANE-NATIVE layout -- element (register n, thread t) at [n][t] -- so every wave
// load/store is one contiguous 1 KiB (s: float4 = (s1, s1', s2, s2') of the lane's 2 pixels).
//
// Per iteration (state: S = line spectra of v = H^T y + rho D^T w):
//   column phase  (x2 halves) rows -> LDS; per column 8 threads: 32-pt FFT in registers, twiddle,
//                 wave-local LDS exchange, radix-8; x C/(MN) (x-update, ops.jl:86); inverse the same
//                 way; LDS -> rows.  Column k = 0 holds the packed real pair (X[0], X[M/2]) and is
//                 separated with its mirror bin (as column_kernel does).
//   line inverse  -> x (registers, lane A pixels 4n,4n+1 / lane B 4n+2,4n+3)
//   row update    s = Dx + clip(s_old) (ops.jl:87-92 with u = clip(s)), w = z - u = phi(s),
//                 v = H^T y + rho D^T w.  Neighbours along dim 1 come from the partner lane (DPP),
//                 along dim 2 from lanes +-2 (ds_bpermute) and, across waves, from two LDS boundary
//                 buffers (x of each wave's last line, w1 of each wave's first line).
//   line forward  -> S
// With a PSF the block first forms H^T y = F^-1 conj(Sigma_c) F y (ops.jl:71-81) the same way.
#include "line_pair.hpp"
#include "plane_api.hpp"

namespace admm {
namespace plane {

constexpr int kPT = 512;                 // threads per block
constexpr int kCS = 264;                 // column stride (float2) in the column buffer; 264 = 8 mod 32
constexpr int kTQ = 33;                  // twiddle-table / exchange row stride (float2)
constexpr int kColF2 = 64 * kCS;         // 64 columns (one half) x 256 bins
constexpr int kTwF2 = 8 * kTQ;
constexpr int kMirF2 = 256;
constexpr int kBndF2 = 8 * 2 * 64;       // 8 waves x 2 lanes x 64 registers
constexpr int kDumF2 = 8 * 128;          // per-wave sink for the branch-free boundary stores
constexpr int kC0F2 = 128;               // (c0 - cL)/2 of the packed column, 256 floats (LDS copy of C0b)
// mir (column phase, half 0) and the sink (row phase) never live at the same time: aliased.
constexpr size_t kLdsBytes = (size_t)(kColF2 + kTwF2 + 2 * kBndF2 + kDumF2 + kC0F2) * 8;
static_assert(kLdsBytes <= 160 * 1024, "LDS budget");
static_assert(kMirF2 <= kDumF2, "mirror buffer aliases the sink");
constexpr int kTab = 2 * 32 * kPT;       // lane-native spectral table entries (= 256 x 128)

// Buffer access with the per-register offset in an SGPR (soffset): element (n, t) of a lane-native
// array is voffset = t * size + soffset = n * 512 * size.  With plain global addressing every n needs
// its own 64-bit VGPR address (the offsets exceed the 13-bit immediate), which costs ~128 VGPRs.
using rsrc_t = __amdgpu_buffer_rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
// AUX: cache-policy bits of the access (gfx950: 1 = sc0, 2 = nt, 16 = sc1); every product access uses the default
// policy (nt / sc0 / sc1 on the s and H^T y streams were measured, round 2: no gain)
template <int AUX = 0>
__device__ __forceinline__ float4 bld4(rsrc_t r, unsigned vo, unsigned so) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, vo, so, AUX));
}
template <int AUX = 0>
__device__ __forceinline__ float2 bld2(rsrc_t r, unsigned vo, unsigned so) {
    return __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(r, vo, so, AUX));
}
__device__ __forceinline__ float bld1(rsrc_t r, unsigned vo, unsigned so) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, vo, so, 0));
}
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
template <int AUX = 0>
__device__ __forceinline__ void bst4(rsrc_t r, unsigned vo, unsigned so, float4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, vo, so, AUX);
}
__device__ __forceinline__ void bst2(rsrc_t r, unsigned vo, unsigned so, float2 v) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, vo, so, 0);
}
__device__ __forceinline__ unsigned bldu(rsrc_t r, unsigned vo, unsigned so) {
    return __builtin_amdgcn_raw_buffer_load_b32(r, vo, so, 0);
}
__device__ __forceinline__ void bstu(rsrc_t r, unsigned vo, unsigned so, unsigned v) {
    __builtin_amdgcn_raw_buffer_store_b32(v, r, vo, so, 0);
}


// Mask-bit trajectory (record mode 2: the reverse sweep will not form rho_bar, so it needs only the ST
// branch of every s_k element, not s_k itself).  Per element c of a lane's register n (float4 (s1, s1', s2,
// s2')) one byte: bits 0-3 = 1[|s_c| > tau], bits 4-7 = sign bit of s_c; 4 registers per dword, stored
// lane-native [n / 4][t]: 32 KiB per plane and iteration instead of 512 KiB of s_k.
__device__ __forceinline__ unsigned mask_byte(float4 s, float tau) {
    const unsigned m = (unsigned)(fabsf(s.x) > tau) | ((unsigned)(fabsf(s.y) > tau) << 1) |
                       ((unsigned)(fabsf(s.z) > tau) << 2) | ((unsigned)(fabsf(s.w) > tau) << 3);
    const unsigned g = (__float_as_uint(s.x) >> 31) | ((__float_as_uint(s.y) >> 31) << 1) |
                       ((__float_as_uint(s.z) >> 31) << 2) | ((__float_as_uint(s.w) >> 31) << 3);
    return m | (g << 4);
}
constexpr unsigned kMaskSlotBytes = 16 * 512 * 4;   // one plane, one iteration

// Fine-grained phase stamps (devtest timing builds only: -DPLANE_TS).
#ifdef PLANE_TS
__device__ unsigned long long* g_plane_ts;
#define PLANE_STAMP(slot)                                                                              \
    do {                                                                                               \
        if ((threadIdx.x & 63) == 0)                                                                   \
            g_plane_ts[((size_t)blockIdx.x * 8 + (threadIdx.x >> 6)) * 64 + (slot)] += __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define PLANE_STAMP(slot) \
    do {                  \
    } while (0)
#endif

// LDS exchange between lanes of one wave: LDS executes a wave's instructions in order, the wait
// makes the dependency explicit and the clobber keeps the compiler from reordering around it.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Block barrier for LDS hand-offs only.  __syncthreads() carries a workgroup release fence that
// waits vmcnt(0), i.e. for every outstanding global store (the s state) to drain before the barrier
// -- which made the store traffic synchronous.  No data moves between threads through global memory
// in this kernel (each thread re-reads only its own lane-native s / H^T y), so LDS ordering suffices.
__device__ __forceinline__ void lds_barrier() {
    __asm__ volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// The prox arithmetic: clip = med3(v, -tau, tau) (one v_med3_f32); w = s - 2 clip(s) as one FMA -- the same values
// as min(max(v, -tau), tau) and |s| > tau ? s - 2 tau sign(s) : -s for every finite input (exact: s - 2s = -s,
// s - 2 tau sign(s) has one rounding either way).  The compare / select form ran c2 at 3.34 ms, this one 3.29 ms
// once the store-data hazard it exposed was padded at build time (hazard_pad.py; census green).
__device__ __forceinline__ float clip_tau(float v, float tau) { return __builtin_amdgcn_fmed3f(v, -tau, tau); }
// w = z - u with z = ST(s, tau) and u = s - z  (|s| > tau: s - 2 tau sign s, else -s)
__device__ __forceinline__ float phi_tau(float s, float tau) { return fmaf(-2.0f, clip_tau(s, tau), s); }

// Materialise every S register at a phase boundary.  Without it the compiler moves the tail of a line
// transform past the next phase's LDS traffic in straight-line code, and the overlap of the two register
// peaks spills (the isotropic kernel: 376 B per lane; inside plane256_kernel's loop the back-edge separates
// them, except in the PSF prologue).
__device__ __forceinline__ void pin_regs(float2 (&S)[64]) {
#pragma unroll
    for (int n = 0; n < 64; ++n) __asm__ volatile("" : "+v"(S[n].x), "+v"(S[n].y));
}

// Lane-native spectral tables, built once per call from the 2-pass tables Ct/Gt (bin (kj, k) at
// kj*(M/2+1) + k).  Entry ((half*4 + i)*8 + q2)*512 + t is the multiplier thread t applies to bin
// kj = q + 8 i + 32 q2 (q = t & 7) of spectral column k = 32 half + (c >> 1) + 64 (c & 1), c = t >> 3.
// Column 0 (packed X[0] / X[M/2] pair): Cf = (c0 + cL)/2 and C0b[kj] = (c0 - cL)/2 (same for G).
__device__ __forceinline__ void tables_body(const float* __restrict__ Ct, const float2* __restrict__ Gt,
                                            float* __restrict__ Cf, float* __restrict__ C0b,
                                            float2* __restrict__ Gf, float2* __restrict__ G0b) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= kTab) return;
    const int t = idx & 511, q2 = (idx >> 9) & 7, i = (idx >> 12) & 3, half = idx >> 14;
    const int q = t & 7, c = t >> 3;
    const int kj = q + 8 * i + 32 * q2;
    const int H = 129;
    if (half == 0 && c == 0) {
        const float c0 = Ct[kj * H], cL = Ct[kj * H + 128];
        Cf[idx] = 0.5f * (c0 + cL);
        C0b[kj] = 0.5f * (c0 - cL);
        if (Gt) {
            const float2 g0 = Gt[kj * H], gL = Gt[kj * H + 128];
            Gf[idx] = cscale(cadd(g0, gL), 0.5f);
            G0b[kj] = cscale(csub(g0, gL), 0.5f);
        }
    } else {
        const int k = 32 * half + (c >> 1) + 64 * (c & 1);
        Cf[idx] = Ct[kj * H + k];
        if (Gt) Gf[idx] = Gt[kj * H + k];
    }
}
__global__ __launch_bounds__(256) void tables_kernel(const float* __restrict__ Ct, const float2* __restrict__ Gt,
                                                     float* __restrict__ Cf, float* __restrict__ C0b,
                                                     float2* __restrict__ Gf, float2* __restrict__ G0b) {
    tables_body(Ct, Gt, Cf, C0b, Gf, G0b);
}
// One half of the column phase: spectral columns k with register m in [32 HALF, 32 HALF + 32).
// MODE 0: real multiplier Cf (x-update); MODE 1: complex multiplier Gf (H^T y).
template <int MODE, int HALF>
__device__ __forceinline__ void column_half(float2 (&S)[64], float2* colbuf, const float2* tw,
                                            float2* mir, rsrc_t Cf, const float* C0b,
                                            rsrc_t Gf, const float2* __restrict__ G0b, int t, bool hb) {
    const int r = t >> 1;
    const int q = t & 7, c = t >> 3;
    PLANE_STAMP(HALF * 8 + 0);
    // rows -> LDS: column c = 2 m + hb holds register 32 HALF + m of every line.  Two bases (m < 16,
    // m >= 16) keep every access base + 16-bit immediate (m * 4224 B would overflow one base).
    float2* rlo = colbuf + hb * kCS + r;
    float2* rhi = rlo + 32 * kCS;
#pragma unroll
    for (int m = 0; m < 16; ++m) rlo[2 * m * kCS] = S[32 * HALF + m];
#pragma unroll
    for (int m = 0; m < 16; ++m) rhi[2 * m * kCS] = S[32 * HALF + 16 + m];
    PLANE_STAMP(HALF * 8 + 1);
    lds_barrier();
    PLANE_STAMP(HALF * 8 + 2);
    float2* col = colbuf + c * kCS;
    const float2* twq = tw + q * kTQ;
    float2 v[32];
    // forward 256 = 32 (in registers, samples j = 8 n + q) x 8 (across the column's 8 lanes)
#pragma unroll
    for (int n = 0; n < 32; ++n) v[n] = col[8 * n + q];
    fft_reg<32, false>(v);
    PLANE_STAMP(HALF * 8 + 3);
#pragma unroll
    for (int k = 0; k < 32; ++k) col[q * kTQ + k] = cmul(v[k], twq[k]);
    // multipliers for this thread's 32 bins (coalesced, L2-resident), issued once v is dead so they do
    // not add to the register peak of the FFT
    sched_fence();
    // MODE 1 (H^T y, once per solve) loads its complex multipliers in two halves of 16: all 32 at once (64 VGPRs)
    // set the PSF kernel's register peak and its allocation spilled inside the iteration loop as well
#ifdef ADMM_PK_F32
    // packed build: the real multipliers too (their 32 VGPRs sit on the dft<8> peak, whose packed temporaries need
    // aligned pairs: the reverse sweep's column phase went from 220 to 252 live VGPRs and spilled)
    constexpr int NGF = 16;
#else
    constexpr int NGF = MODE == 1 ? 16 : 32;
#endif
    float cf[MODE == 0 ? NGF : 1];
    float2 gf[MODE == 1 ? 32 : 1];
#pragma unroll
    for (int j = 0; j < NGF; ++j) {
        if constexpr (MODE == 0) cf[j] = bld1(Cf, t * 4, (HALF * 32 + j) * kPT * 4);
        else gf[j] = bld2(Gf, t * 8, (HALF * 32 + j) * kPT * 8);
    }
    wave_lds_sync();
    float2 u[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int qq = 0; qq < 8; ++qq) u[i][qq] = col[qq * kTQ + q + 8 * i];
        dft<8, false>(u[i]);
    }
    PLANE_STAMP(HALF * 8 + 4);
    // u[i][q2] = bin kj = q + 8 i + 32 q2 of this column.
    // Column k = 0 carries the packed real pair (X[0], X[M/2]): x(c0+cL)/2 plus (c0-cL)/2 x conj(Z(-kj))
    // separates them (column_kernel's mirror form).  The mirror bin lives in another lane of the same
    // column, so wave 0 (columns 0..7) swaps the raw bins through LDS.  The branches are wave-uniform
    // and the other lanes' stores go to a dummy region: no lane diverges.
    // wave-uniform (readfirstlane makes it a scalar branch, not an EXEC mask)
    const bool wave0 = HALF == 0 && __builtin_amdgcn_readfirstlane(t >> 6) == 0;
    const bool col0 = c == 0;
    if (wave0) {
        // bin kj of column 0 goes to mir[kj]; bin 0 also to mir[256] so that the mirror read below,
        // mir[256 - kj] = mir[(8 - q) + 8 (3 - i) + 32 (7 - q2)], is a lane base + immediate offsets
        float2* mw = col0 ? mir + q : mir + 512 + q;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q2 = 0; q2 < 8; ++q2) mw[8 * i + 32 * q2] = u[i][q2];
        float2* m256 = (col0 && q == 0) ? mir + 256 : mir + 520 + (t & 63);   // others: dummy slots
        *m256 = u[0][0];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if constexpr (NGF == 16) {
            if (i == 2) {   // second half of the multipliers, into the slots of the first
                sched_fence();
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    if constexpr (MODE == 0) cf[j] = bld1(Cf, t * 4, (HALF * 32 + 16 + j) * kPT * 4);
                    else gf[j] = bld2(Gf, t * 8, (HALF * 32 + 16 + j) * kPT * 8);
                }
            }
        }
#pragma unroll
        for (int q2 = 0; q2 < 8; ++q2) {
            if constexpr (MODE == 0) u[i][q2] = cscale(u[i][q2], cf[(i * 8 + q2) % NGF]);
            else u[i][q2] = cmul(u[i][q2], gf[(i * 8 + q2) % NGF]);
        }
    }
    if (wave0) {
        wave_lds_sync();
        const float2* mr = mir + (8 - q);
        const float* c0q = C0b + q;
        const float2* g0q = G0b + q;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q2 = 0; q2 < 8; ++q2) {
                const float2 zm = cconj(mr[8 * (3 - i) + 32 * (7 - q2)]);
                float2 add;
                if constexpr (MODE == 0) add = cscale(zm, c0q[8 * i + 32 * q2]);
                else add = cmul(zm, g0q[8 * i + 32 * q2]);
                u[i][q2].x += col0 ? add.x : 0.0f;
                u[i][q2].y += col0 ? add.y : 0.0f;
            }
    }
    PLANE_STAMP(HALF * 8 + 5);
    // inverse: radix-8 across lanes, exchange, twiddle, 32-pt IFFT
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        dft<8, true>(u[i]);
#pragma unroll
        for (int qq = 0; qq < 8; ++qq) col[qq * kTQ + q + 8 * i] = u[i][qq];
    }
    wave_lds_sync();
#pragma unroll
    for (int k = 0; k < 32; ++k) v[k] = cmul(col[q * kTQ + k], cconj(twq[k]));
    fft_reg<32, true>(v);
#pragma unroll
    for (int n = 0; n < 32; ++n) col[8 * n + q] = v[n];
    PLANE_STAMP(HALF * 8 + 6);
    lds_barrier();
    PLANE_STAMP(HALF * 8 + 7);
#pragma unroll
    for (int m = 0; m < 16; ++m) S[32 * HALF + m] = rlo[2 * m * kCS];
#pragma unroll
    for (int m = 0; m < 16; ++m) S[32 * HALF + 16 + m] = rhi[2 * m * kCS];
    lds_barrier();
}

// Line r -/+ 1 of the lane-pair layout is lane t -/+ 2: two whole-wave DPP shifts (wave_shr:1 / wave_shl:1, VALU)
// per value (a __shfl_up / __shfl_down is a ds_bpermute, an LDS round trip on the row phase's dependency chain:
// c2 3.284 -> 3.259 ms).  Lanes 0,1 (up) / 62,63 (down) receive 0; the callers overwrite them with the boundary
// lines from LDS.
// v is pinned in place (the caller's own variable, which it reads again): pinning a by-value copy kept the
// original alive beside it, one v_mov per shift
__device__ __forceinline__ float lane_up2(float& vr) {   // lane i <- lane i - 2
    float v = vr;
    __asm__ volatile("" : "+v"(v));
    const int a = __builtin_amdgcn_mov_dpp(__float_as_int(v), 0x138, 0xF, 0xF, true);
    return __int_as_float(__builtin_amdgcn_mov_dpp(a, 0x138, 0xF, 0xF, true));
}
__device__ __forceinline__ float lane_down2(float& vr) {   // lane i <- lane i + 2
    float v = vr;
    __asm__ volatile("" : "+v"(v));
    const int a = __builtin_amdgcn_mov_dpp(__float_as_int(v), 0x130, 0xF, 0xF, true);
    return __int_as_float(__builtin_amdgcn_mov_dpp(a, 0x130, 0xF, 0xF, true));
}

// v(register n) = H^T y + rho D^T w, with w of registers n and n+1 (the partner lane's pixel after this
// lane's last pixel lives one register later on lane A).
// The wave's last line (lanes 62, 63) has no source lane in the two shifts: lane_down2 leaves +0 there (bound_ctrl), which
// is what the sum needs until the next wave's first line is fixed up after the barrier -- no select on the lane.
__device__ __forceinline__ float2 finalize(float4 wn, float4 wnext, float2 hy, bool hb, float rho) {
    const float recv = swapf(hb ? wn.z : wnext.z);     // w2 at the pixel after this lane's 2nd pixel
    const float w1x = lane_down2(wn.x), w1y = lane_down2(wn.y);   // w1 of line r+1; 0 on the wave's last line
    const float q0 = wn.x - w1x + wn.z - wn.w;
    const float q1 = wn.y - w1y + wn.w - recv;
    return make_float2(fmaf(rho, q0, hy.x), fmaf(rho, q1, hy.y));
}

// x (spatial, registers) -> s_k = Dx + clip(s_{k-1}) stored, S <- v = H^T y + rho D^T phi(s_k).
// Branch-free inside: the boundary-line LDS traffic is done by every lane (reads broadcast from two
// addresses, writes of non-boundary lanes go to a per-thread sink) so the chunk loop stays one block.
// first: iteration 1, s_{k-1} = 0 (ops.jl:48-49 zero init): the caller passes a resource of size 0 for sp then,
// whose loads return 0 (clip(0) = 0), so one copy of this code serves every iteration without a select.
//
// Register budget: S (128 VGPRs) is the bulk.  The column buffer is idle here, so x of registers
// 32..63 is parked in it (per-lane slots stg[m * 512 + t]) while registers 0..31 are processed; at
// the half-way point the slots swap x[32+m] back in and v[m] out, and v[0..30] return at the end.
// The chunk loop thus holds ~66 S registers instead of 128.
// STAGED: the line inverse already parked x of registers 32..63 in the staging slots
// (line_inverse_pair_staged); S[32..63] are dead on entry.
template <bool STAGED = false, bool MASK = false>
__device__ __forceinline__ void row_update(float2 (&S)[64], rsrc_t sp, rsrc_t sps, rsrc_t hp, float2* xb,
                                           float2* wb, float2* sink, float2* colbuf, int t, bool hb, bool first,
                                           float tau, float rho, rsrc_t mrs) {
    (void)first;
#ifndef PLANE_CH
#define PLANE_CH 2
#endif
    constexpr int CH = PLANE_CH;     // registers per chunk
#ifndef PLANE_PD
#define PLANE_PD 2
#endif
    // Prefetch distance (chunks in flight).  Round 1's PD > 1 builds hit the store-data hazard that
    // hazard_pad.py now pads; padded, PD = 2 passes the census and is the fastest
    // (c2 3.31 -> 3.20 ms; PD = 3 3.22, CH = 4 3.21).
    constexpr int PD = PLANE_PD;
    constexpr int NCH = 64 / CH;
    const int lane = t & 63, w = t >> 6;
    const bool top = lane < 2, bot = lane >= 62;
    // ring of PD+1 chunk buffers of s_{k-1} and H^T y (compile-time slots: the chunk loop is unrolled)
    float4 sor[PD + 1][CH];
    float2 hyr[PD + 1][CH];
    PLANE_STAMP(16);
    // staging slots stg[m * 512 + t]: two bases keep the offsets within the 16-bit ds immediate
    float2* stg = colbuf + t;
    float2* stg2 = stg + 16 * kPT;
    float x63y;   // lane A's register 0 needs the pixel before it (B's pixel 255)
    if constexpr (STAGED) {
        if (bot) {
#pragma unroll
            for (int n = 0; n < 32; ++n) xb[(w * 2 + hb) * 64 + n] = S[n];
#pragma unroll
            for (int m = 0; m < 16; ++m) xb[(w * 2 + hb) * 64 + 32 + m] = stg[m * kPT];
#pragma unroll
            for (int m = 0; m < 16; ++m) xb[(w * 2 + hb) * 64 + 48 + m] = stg2[m * kPT];
        }
        x63y = stg2[15 * kPT].y;
    } else {
        if (bot) {
#pragma unroll
            for (int n = 0; n < 64; ++n) xb[(w * 2 + hb) * 64 + n] = S[n];
        }
        x63y = S[63].y;
#pragma unroll
        for (int m = 0; m < 16; ++m) stg[m * kPT] = S[32 + m];
#pragma unroll
        for (int m = 0; m < 16; ++m) stg2[m * kPT] = S[48 + m];
    }
    lds_barrier();
    // prologue loads after the staging: issued earlier they made every spill reload around the line
    // inverse wait for them (one in-order vmcnt)
    sched_fence();
#pragma unroll
    for (int g = 0; g < PD; ++g)
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            sor[g][j] = bld4(sp, t * 16, (g * CH + j) * kPT * 16);
            hyr[g][j] = bld2(hp, t * 8, (g * CH + j) * kPT * 8);
        }
    PLANE_STAMP(17);
    const float2* xbp = xb + (((w + 7) & 7) * 2 + hb) * 64;   // previous wave's last line
    // this wave's first line (w1); the other lanes write garbage to sink[w][lane + n] (distinct
    // addresses per instruction, same immediate offsets as the real stores)
    float2* wbm = top ? wb + (w * 2 + hb) * 64 : sink + w * 128 + lane;
    float4 wc[CH + 1];
    float2 hc[CH + 1];
    float w2x0 = 0.0f;
    unsigned mbits = 0;   // MASK: the bytes of registers 4 (n / 4) .. n
#pragma unroll
    for (int g = 0; g < NCH; ++g) {
        const int n0 = g * CH;
        if (g + PD < NCH) {
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                // keep the slot's old value live up to here, so its registers are not recycled as
                // temporaries (and read by VALU/DPP) just before this load overwrites them
                __asm__ volatile("" ::"v"(sor[(g + PD) % (PD + 1)][j].x), "v"(sor[(g + PD) % (PD + 1)][j].y),
                                 "v"(sor[(g + PD) % (PD + 1)][j].z), "v"(sor[(g + PD) % (PD + 1)][j].w),
                                 "v"(hyr[(g + PD) % (PD + 1)][j].x), "v"(hyr[(g + PD) % (PD + 1)][j].y));
                sor[(g + PD) % (PD + 1)][j] = bld4(sp, t * 16, ((g + PD) * CH + j) * kPT * 16);
                hyr[(g + PD) % (PD + 1)][j] = bld2(hp, t * 8, ((g + PD) * CH + j) * kPT * 8);
            }
        }
        if (n0 == 32) {   // half-way: x[32..63] in, v[0..30] out (x[31] still pending in S[31])
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const float2 xv = stg[m * kPT];
                stg[m * kPT] = S[m];
                S[32 + m] = xv;
            }
#pragma unroll
            for (int m = 0; m < 15; ++m) {
                const float2 xv = stg2[m * kPT];
                stg2[m * kPT] = S[16 + m];
                S[48 + m] = xv;
            }
            S[63] = stg2[15 * kPT];
            sched_fence();
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int n = n0 + j;
            const float4 so = sor[g % (PD + 1)][j];
            float2 x = S[n];
            const float xl = swapf(hb ? (n == 0 ? x63y : S[(n + 63) & 63].y) : x.y);   // pixel before this lane's first
            const float2 xub = xbp[n];
            float2 xu = make_float2(lane_up2(x.x), lane_up2(x.y));   // line r-1
            xu.x = top ? xub.x : xu.x;
            xu.y = top ? xub.y : xu.y;
            // iteration 1 (first): so comes from a resource of size 0 (the caller's), i.e. 0, and clip(0) = 0: no select
            float4 uo = make_float4(clip_tau(so.x, tau), clip_tau(so.y, tau), clip_tau(so.z, tau), clip_tau(so.w, tau));
            if (first) uo = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 s = make_float4(x.x - xu.x + uo.x, x.y - xu.y + uo.y, x.x - xl + uo.z, x.y - x.x + uo.w);
            bst4(sps, t * 16, n * kPT * 16, s);
            if constexpr (MASK) {
                mbits |= mask_byte(s, tau) << (8 * (n & 3));
                if ((n & 3) == 3) {
                    bstu(mrs, t * 4, (n >> 2) * kPT * 4, mbits);
                    mbits = 0;
                }
            }
            wc[j + 1] = make_float4(phi_tau(s.x, tau), phi_tau(s.y, tau), phi_tau(s.z, tau), phi_tau(s.w, tau));
            hc[j + 1] = hyr[g % (PD + 1)][j];
            wbm[n] = make_float2(wc[j + 1].x, wc[j + 1].y);
            sched_fence();
        }
        if (g == 0) w2x0 = wc[1].z;
#pragma unroll
        for (int j = (g == 0 ? 1 : 0); j < CH; ++j) {
            S[n0 - 1 + j] = finalize(wc[j], wc[j + 1], hc[j], hb, rho);
            sched_fence();
        }
        wc[0] = wc[CH];
        hc[0] = hc[CH];
        sched_fence();
    }
    S[63] = finalize(wc[0], make_float4(0.f, 0.f, w2x0, 0.f), hc[0], hb, rho);
#pragma unroll
    for (int m = 0; m < 16; ++m) S[m] = stg[m * kPT];
#pragma unroll
    for (int m = 0; m < 15; ++m) S[16 + m] = stg2[m * kPT];
    PLANE_STAMP(18);
    lds_barrier();
    PLANE_STAMP(19);
    if (bot) {
        const float2* wbn = wb + (((w + 1) & 7) * 2 + hb) * 64;   // next wave's first line
#pragma unroll
        for (int n = 0; n < 64; ++n) {
            const float2 a = wbn[n];
            S[n].x = fmaf(-rho, a.x, S[n].x);
            S[n].y = fmaf(-rho, a.y, S[n].y);
        }
    }
}

template <int MODE>
__device__ __forceinline__ void column_phase(float2 (&S)[64], float2* colbuf, const float2* tw, float2* mir,
                                             rsrc_t Cf, const float* C0b, rsrc_t Gf, const float2* G0b,
                                             int t, bool hb) {
    column_half<MODE, 0>(S, colbuf, tw, mir, Cf, C0b, Gf, G0b, t, hb);
    column_half<MODE, 1>(S, colbuf, tw, mir, Cf, C0b, Gf, G0b, t, hb);
}

// debug aid (devtest only): DBG == 1 dumps S after each phase of every iteration (plane 0);
// DBG == 2 records the shader clock at each phase boundary (lane 0 of every wave, every plane);
// DBG == 3 only the workgroup start / end (slots 508 / 509), otherwise the product kernel.
template <int DBG>
__device__ __forceinline__ void dbg_dump(float2* dbg, const float2 (&S)[64], int slot, int t) {
    if constexpr (DBG == 2) {
        if ((t & 63) == 0) {
            const unsigned long long c = __builtin_amdgcn_s_memtime();
            reinterpret_cast<unsigned long long*>(dbg)[((size_t)blockIdx.x * 8 + (t >> 6)) * 512 + slot] = c;
        }
    } else if constexpr (DBG == 1) {
        if (blockIdx.x == 0) {
#pragma unroll
            for (int n = 0; n < 64; ++n) dbg[((size_t)slot * 64 + n) * kPT + t] = S[n];
        }
    }
}


// grid = planes, block = 512, dynamic LDS = kLdsBytes.  K >= 1.
// TRAJ: record the trajectory for the adjoint -- iteration k writes s_k to slot k-1 of `traj` (slot
// stride traj_slot float4, lane-native layout, plane p at p * 64 * 512) and reads s_{k-1} from slot
// k-2, instead of updating sln in place.  Same bytes per iteration as the plain solve.
// TRAJ 2: record the ST mask bits of s_k instead (mask_byte): s stays in place in sln as in the plain solve,
// and iteration k writes its mask slot k-1 (mtraj + (k-1) * mslot dwords, plane p at p * 16 * 512).
// TRAJ 3: the state instance of the resumable solve (plane_state.hip).  s stays in place in sln and s_{K-1} is stored
// (the store resource stays live for every k <= K - 1, as in TRAJ 1): the end kernel forms s_K from it.  mtraj, when set,
// is not a mask trajectory but v_0 = rho D^T (z_0 - u_0) of a warm start (floats, natural layout, a plane 65536 apart):
// it joins H^T y before the first line transform, sln then holds s_0 (state_import_kernel) and iteration 1 reads it
// with the full-size resource and first = false.  mtraj NULL: the cold start, zero-size resource at k = 1 as above.
// br: several branches in one grid (Branches; nbr = 1 is a single solve).
// GRP: a grouped solve (br.nbr = 0): plane q reads and writes plane q with the tables and scalars of group_of(q).
template <bool PSF, int DBG = 0, int TRAJ = 0, bool GRP = false>
__global__ __launch_bounds__(kPT) void plane256_kernel(const float* __restrict__ y, float* __restrict__ x_out,
                                                       const float* __restrict__ Cf, const float* __restrict__ C0b,
                                                       const float2* __restrict__ Gf, const float2* __restrict__ G0b,
                                                       float2* __restrict__ hln, float4* __restrict__ sln, const float* __restrict__ prm, int K, float2* dbg = nullptr,
                                                       float4* __restrict__ traj = nullptr, size_t traj_slot = 0,
                                                       Branches br = Branches{1, 1, 1, 0u, 0u},
                                                       unsigned* __restrict__ mtraj = nullptr, size_t mslot = 0) {
    const BranchOf bo = plane_of<GRP>(br, blockIdx.x);
    Cf += (size_t)bo.i * br.tab_f;
    C0b += (size_t)bo.i * br.tab_f;
    Gf = reinterpret_cast<const float2*>(reinterpret_cast<const float*>(Gf) + (size_t)bo.i * br.tab_f);
    G0b = reinterpret_cast<const float2*>(reinterpret_cast<const float*>(G0b) + (size_t)bo.i * br.tab_f);
    prm += (size_t)bo.i * br.prm_f;
    const float tau = prm[0]; const float rho = prm[1];   // device-resident scalars (setup_kernel)
    if constexpr (DBG >= 2) {   // workgroup start / end on the constant 100 MHz clock (slots 508 / 509 of wave 0)
        if (threadIdx.x == 0)
            reinterpret_cast<unsigned long long*>(dbg)[(size_t)blockIdx.x * 8 * 512 + 508] = __builtin_amdgcn_s_memrealtime();
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2* colbuf = reinterpret_cast<float2*>(smem_raw);
    float2* tw = colbuf + kColF2;
    float2* xb = tw + kTwF2;
    float2* wb = xb + kBndF2;
    float2* sink = wb + kBndF2;
    float2* mir = sink;
    const int t = threadIdx.x;
    float* c0l = reinterpret_cast<float*>(sink + kDumF2);   // C0b, read by wave 0 in every column phase
    if (t < 256) c0l[t] = C0b[t];                             // visible after the first barrier
    const bool hb = t & 1;
    const int r = t >> 1;
    const size_t plane = blockIdx.x;
    if (t < 256) {   // W256^(q k), q = 0..7, k = 0..31 (visible after the first barrier)
        const int q = t >> 5, k = t & 31;
        double sn, cs;
        sincospi((double)(q * k) / 128.0, &sn, &cs);
        tw[q * kTQ + k] = make_float2((float)cs, (float)-sn);
    }
    const float2* yrow = reinterpret_cast<const float2*>(y + bo.in_plane * 65536 + (size_t)r * 256);
    float2 S[64];
#pragma unroll
    for (int n = 0; n < 64; ++n) S[n] = yrow[2 * n + hb];
    const rsrc_t hp = make_rsrc(hln + plane * kHtyStrideF2, 64 * kPT * 8);
    const rsrc_t sp = make_rsrc(sln + plane * 64 * kPT, 64 * kPT * 16);
    const rsrc_t cfr = make_rsrc(Cf, kTab * 4);
    const rsrc_t gfr = make_rsrc(Gf, PSF ? kTab * 8 : 0);
    if constexpr (PSF) {
        line_forward_pair(S, hb);
        pin_regs(S);
        column_phase<1>(S, colbuf, tw, mir, cfr, C0b, gfr, G0b, t, hb);
        // = H^T y (the 1/(MN) is in Gf).  Staged as in the iterations (x[32..63] through per-thread LDS
        // slots, no barrier): the unstaged inverse's peak exceeds 256 VGPRs and spilled.
        line_inverse_pair_staged(S, hb, colbuf + t, colbuf + t + 16 * kPT);
#pragma unroll
        for (int m = 0; m < 32; ++m) S[32 + m] = colbuf[t + m * kPT];
    }
#pragma unroll
    for (int n = 0; n < 64; ++n) bst2(hp, t * 8, n * kPT * 8, S[n]);
    if constexpr (TRAJ == 3) {
        if (mtraj) {   // warm start: v = H^T y + v_0, a natural-layout row read like yrow
            const float2* vrow = reinterpret_cast<const float2*>(reinterpret_cast<const float*>(mtraj) +
                                                                 plane * 65536 + (size_t)r * 256);
#pragma unroll
            for (int n = 0; n < 64; ++n) {
                const float2 a = vrow[2 * n + hb];
                S[n].x += a.x;
                S[n].y += a.y;
            }
        }
    }
    line_forward_pair(S, hb);
    dbg_dump<DBG>(dbg, S, 0, t);
    for (int k = 1;; ++k) {
        column_half<0, 0>(S, colbuf, tw, mir, cfr, c0l, gfr, G0b, t, hb);
        if constexpr (DBG == 2) dbg_dump<DBG>(dbg, S, 256 + k, t);
        column_half<0, 1>(S, colbuf, tw, mir, cfr, c0l, gfr, G0b, t, hb);
        dbg_dump<DBG>(dbg, S, 4 * k - 3, t);
        // the last iteration keeps x in registers for the output; the others hand x[32..63] to the
        // row phase's LDS staging slots directly (no spill of the line inverse's peak)
        constexpr bool kStage = DBG == 0 || DBG == 3;
        if constexpr (!kStage) {
            line_inverse_pair(S, hb);
            dbg_dump<DBG>(dbg, S, 4 * k - 2, t);
            if (k == K) break;
        } else {
            line_inverse_pair_staged(S, hb, colbuf + t, colbuf + t + 16 * kPT);
            if (k == K) {   // the output needs x[32..63] back (per-thread slots: no barrier)
#pragma unroll
                for (int m = 0; m < 16; ++m) S[32 + m] = colbuf[t + m * kPT];
#pragma unroll
                for (int m = 0; m < 16; ++m) S[48 + m] = colbuf[t + (16 + m) * kPT];
                break;
            }
        }
        // iteration 1 has no s_0 to read (zero init, ops.jl:48-49): its loads go to a resource of size 0,
        // which returns zeros without touching memory
        if constexpr (TRAJ == 1) {
            float4* tb = traj + plane * 64 * kPT;
            const rsrc_t sld = make_rsrc(tb + (size_t)(k >= 2 ? k - 2 : 0) * traj_slot, k >= 2 ? 64 * kPT * 16 : 0);
            const rsrc_t sst = make_rsrc(tb + (size_t)(k - 1) * traj_slot, 64 * kPT * 16);
            row_update<kStage>(S, sld, sst, hp, xb, wb, sink, colbuf, t, hb, k == 1, tau, rho, sld);
        } else if constexpr (TRAJ == 2) {
            // s in place as below (s_{K-1} is not stored: only its mask bits are needed after the solve)
            const rsrc_t sld = k >= 2 ? sp : make_rsrc(sln, 0);
            const rsrc_t sst = k <= K - 2 ? sp : make_rsrc(sln, 0);
            const rsrc_t mrs = make_rsrc(mtraj + (size_t)(k - 1) * mslot + plane * 16 * kPT, kMaskSlotBytes);
            row_update<kStage, true>(S, sld, sst, hp, xb, wb, sink, colbuf, t, hb, k == 1, tau, rho, mrs);
        } else if constexpr (TRAJ == 3) {
            const bool warm = mtraj != nullptr;
            const rsrc_t sld = (k >= 2 || warm) ? sp : make_rsrc(sln, 0);
            row_update<kStage>(S, sld, sp, hp, xb, wb, sink, colbuf, t, hb, k == 1 && !warm, tau, rho, sld);
        } else {
            // ... and s_{K-1} is never read (iteration K stops at x): its stores drop the same way
            const rsrc_t sld = k >= 2 ? sp : make_rsrc(sln, 0);
            const rsrc_t sst = k <= K - 2 ? sp : make_rsrc(sln, 0);
            row_update<kStage>(S, sld, sst, hp, xb, wb, sink, colbuf, t, hb, k == 1, tau, rho, sld);
        }
        dbg_dump<DBG>(dbg, S, 4 * k - 1, t);
        line_forward_pair(S, hb);
        dbg_dump<DBG>(dbg, S, 4 * k, t);
    }
#ifdef ADMM_PK_F32
    // the output row from a thread index taken here: formed from r, its address is computed at the kernel's start and
    // held in a VGPR pair through every phase (the packed build has none to spare: 8 B of scratch per lane)
    int ro = threadIdx.x >> 1;
    __asm__ volatile("" : "+v"(ro));
#else
    const int ro = r;
#endif
    float2* xrow = reinterpret_cast<float2*>(x_out + bo.out_plane * 65536 + (size_t)ro * 256);
#pragma unroll
    for (int n = 0; n < 64; ++n) xrow[2 * n + hb] = S[n];
    if constexpr (DBG >= 2) {
        if (threadIdx.x == 0)
            reinterpret_cast<unsigned long long*>(dbg)[(size_t)blockIdx.x * 8 * 512 + 509] = __builtin_amdgcn_s_memrealtime();
    }
}


// =============================================================================================
// Fused per-plane ADJOINT (reverse sweep of the anisotropic solve): one
// workgroup per 256 x 256 plane runs all K reverse steps with the line spectra in registers, the
// structure of plane256_kernel run backwards (admm_backward.hip's header states the recurrences;
// tests/kernel_model.py tvd_model_grads restates them):
//   S = line spectra of g_K = x_bar
//   step k = K..1:  column phase (x C/(MN): vbar_k = A^-1 g_k, A symmetric), line inverse -> vbar_k,
//                   row phase (row_adjoint), line forward of g_{k-1} = D^T sbar_{k-1} (k >= 2)
// HBM per pixel and step: s_{k-1}, s_k (or D x_K at k = K), sbar_k in, sbar_{k-1} out (8 B each),
// Vsum in + out (4 B each) -- 40 B/px vs 72 for the 2-pass step (line_adj + column round trips of the
// spectrum).  Absent operands (sbar_K, Vsum before step K, s_0, sbar_0) are buffer resources of size 0:
// their loads return 0 and their stores are dropped, so one loop body serves every step.
// =============================================================================================

// Row phase of reverse step k.  v = vbar_k (spatial; registers 32..63 staged by the line inverse).
//   Dvb = D vbar_k (neighbours as x in row_update);  rho_acc -= <Dvb, D x_k>, D x_k = s_k - clip(s_{k-1})
//   (k = K: the precomputed D x_K);  Vsum += vbar_k;
//   wbar = rho Dvb, m = |s_{k-1}| > tau:  sbar_{k-1} = m ? wbar : sbar_k - wbar,
//   rho_acc += <phi(s_{k-1}), Dvb>,  tau_acc += m sgn(s_{k-1}) (sbar_k - 2 wbar);
//   S <- g_{k-1} = D^T sbar_{k-1}  (finalize with H^T y = 0 and unit weight).
// Chunks of ONE register (the ring holds 3 float4 + 1 float2 per register, 2.3x row_update's).
// WV: the running sum Vsum of vbar is kept (y_bar or h_bar wanted); without it no Vsum instruction is issued
// at all (zero-size resources would drop the traffic, but their loads still queue in the in-order vmcnt)
template <bool MASK, bool WV>
__device__ __forceinline__ void row_adjoint(float2 (&S)[64], rsrc_t s1p, rsrc_t s2p, rsrc_t sbl, rsrc_t sbs, rsrc_t vlp,
                                            rsrc_t vsp, unsigned vso, unsigned vss, float2* xb, float2* wb,
                                            float2* sink, float2* colbuf, int t, bool hb, bool lastk, float tau,
                                            float rho, float& racc, float& tacc) {
    const int lane = t & 63, w = t >> 6;
    const bool top = lane < 2, bot = lane >= 62;
#ifndef ADJ_PD
#define ADJ_PD 4
#endif
    // registers of loads in flight ahead of the one being processed: 4 (c5 one-grid reverse sweep 14.38 ->
    // 13.29 ms against 1; 2: 13.78, 3: 13.49, 6: 13.60, 8: 13.42 and scratch in the full-trajectory variant)
    constexpr int PD = ADJ_PD;
    constexpr int NR = PD + 1;   // ring slots
    float4 s1r[NR], s2r[NR], sbr[NR];
    float2 vr[NR];
    unsigned mwr[2];   // MASK: s1p is the mask-bit slot of s_{k-1} (one dword per 4 registers)
    float2* stg = colbuf + t;
    float2* stg2 = stg + 16 * kPT;
    if (bot) {
#pragma unroll
        for (int n = 0; n < 32; ++n) xb[(w * 2 + hb) * 64 + n] = S[n];
#pragma unroll
        for (int m = 0; m < 16; ++m) xb[(w * 2 + hb) * 64 + 32 + m] = stg[m * kPT];
#pragma unroll
        for (int m = 0; m < 16; ++m) xb[(w * 2 + hb) * 64 + 48 + m] = stg2[m * kPT];
    }
    const float v63y = stg2[15 * kPT].y;
    lds_barrier();
    sched_fence();
    if constexpr (MASK) mwr[0] = bldu(s1p, t * 4, 0);
#pragma unroll
    for (int i = 0; i < PD; ++i) {
        if constexpr (!MASK) {
            s1r[i] = bld4(s1p, t * 16, i * kPT * 16);
            s2r[i] = bld4(s2p, t * 16, i * kPT * 16);
        }
        sbr[i] = bld4(sbl, t * 16, i * kPT * 16);
        if constexpr (WV) vr[i] = bld2(vlp, t * 8, i * kPT * 8);
        else vr[i] = make_float2(0.f, 0.f);
    }
    const float2* xbp = xb + (((w + 7) & 7) * 2 + hb) * 64;   // previous wave's last line
    float2* wbm = top ? wb + (w * 2 + hb) * 64 : sink + w * 128 + lane;
    float4 wc[2];
    float w2x0 = 0.0f;
    const float2 zero2 = make_float2(0.0f, 0.0f);
#pragma unroll
    for (int n = 0; n < 64; ++n) {
        if constexpr (MASK) {   // the dword of the next 4 registers, PD registers ahead
            if (n + PD < 64 && ((n + PD) & 3) == 0) mwr[((n + PD) >> 2) & 1] = bldu(s1p, t * 4, ((n + PD) >> 2) * kPT * 4);
        }
        if (n + PD < 64) {
            const int q = (n + PD) % NR;
            if constexpr (!MASK) {
                __asm__ volatile("" ::"v"(s1r[q].x), "v"(s1r[q].y), "v"(s1r[q].z), "v"(s1r[q].w), "v"(s2r[q].x),
                                 "v"(s2r[q].y), "v"(s2r[q].z), "v"(s2r[q].w));
            }
            __asm__ volatile("" ::"v"(sbr[q].x), "v"(sbr[q].y), "v"(sbr[q].z), "v"(sbr[q].w));
            if constexpr (WV) __asm__ volatile("" ::"v"(vr[q].x), "v"(vr[q].y));
            if (!MASK) s1r[q] = bld4(s1p, t * 16, (n + PD) * kPT * 16);
            if (!MASK) s2r[q] = bld4(s2p, t * 16, (n + PD) * kPT * 16);
            sbr[q] = bld4(sbl, t * 16, (n + PD) * kPT * 16);
            if (WV) vr[q] = bld2(vlp, t * 8, (n + PD) * kPT * 8);
        }
        if (n == 32) {   // half-way: vbar[32..63] in, g[0..30] out (vbar[31] still pending in S[31])
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const float2 xv = stg[m * kPT];
                stg[m * kPT] = S[m];
                S[32 + m] = xv;
            }
#pragma unroll
            for (int m = 0; m < 15; ++m) {
                const float2 xv = stg2[m * kPT];
                stg2[m * kPT] = S[16 + m];
                S[48 + m] = xv;
            }
            S[63] = stg2[15 * kPT];
            sched_fence();
        }
        const float4 s1 = MASK ? make_float4(0.f, 0.f, 0.f, 0.f) : s1r[n % NR];
        const float4 s2 = MASK ? make_float4(0.f, 0.f, 0.f, 0.f) : s2r[n % NR];
        const float4 sb = sbr[n % NR];
        const float2 vo = vr[n % NR];
        float2 v = S[n];
        const float vl = swapf(hb ? (n == 0 ? v63y : S[(n + 63) & 63].y) : v.y);
        const float2 vub = xbp[n];
        float2 vu = make_float2(lane_up2(v.x), lane_up2(v.y));
        vu.x = top ? vub.x : vu.x;
        vu.y = top ? vub.y : vu.y;
        const float dv[4] = {v.x - vu.x, v.y - vu.y, v.x - vl, v.y - v.x};
        const float a1[4] = {s1.x, s1.y, s1.z, s1.w}, a2[4] = {s2.x, s2.y, s2.z, s2.w};
        const float b[4] = {sb.x, sb.y, sb.z, sb.w};
        float nb[4];
        if constexpr (MASK) {
            // rho_bar is not formed in this mode (its <D vbar, D x_k> needs s_k itself): only the branch
            // decisions enter -- bitwise the same sbar and tau_bar as from the full trajectory
            // Branch-free by construction (bit selects, no `m ? :`): from per-lane bits the compiler turned the
            // selects into EXEC-masked branches, and the lane shifts (DPP) of neighbouring registers it
            // scheduled into them then read inactive lanes.  Same values as the full path, bit for bit:
            // sbar = m ? wbar : sbar_k - wbar;  tau_acc += m ? sgn (sbar_k - 2 wbar) : 0 (sgn = +-1: a sign flip).
            const unsigned byte = mwr[(n >> 2) & 1] >> (8 * (n & 3));
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float wbv = rho * dv[c];
                const unsigned msk = 0u - ((byte >> c) & 1u);                 // all ones where |s| > tau
                const unsigned sgb = ((byte >> (4 + c)) & 1u) << 31;          // sign bit of s
                const unsigned keep = __float_as_uint(wbv), pass = __float_as_uint(b[c] - wbv);
                nb[c] = __uint_as_float((keep & msk) | (pass & ~msk));
                const unsigned tv = __float_as_uint(b[c] - 2.0f * wbv) ^ sgb;
                tacc += __uint_as_float(tv & msk);
            }
            (void)a1;
            (void)a2;
        } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float dx = lastk ? a2[c] : a2[c] - clip_tau(a1[c], tau);
            racc -= dv[c] * dx;
            const float wbv = rho * dv[c];
            const bool m = fabsf(a1[c]) > tau;
            nb[c] = m ? wbv : b[c] - wbv;
            racc += phi_tau(a1[c], tau) * dv[c];
            const float sg = (a1[c] > 0.f) ? 1.0f : -1.0f;
            tacc += m ? sg * (b[c] - 2.0f * wbv) : 0.0f;
        }
        }
        // pin the accumulators here: left free, the compiler sinks the sums to the end of the
        // unrolled loop and keeps every register's operands live until then (~2000 VGPRs of spills)
        __asm__ volatile("" : "+v"(racc), "+v"(tacc));
        if (WV) bst2(vsp, vso, n * vss, make_float2(vo.x + v.x, vo.y + v.y));
        const float4 nb4 = make_float4(nb[0], nb[1], nb[2], nb[3]);
        bst4(sbs, t * 16, n * kPT * 16, nb4);
        wbm[n] = make_float2(nb4.x, nb4.y);
        if (n == 0) {
            w2x0 = nb4.z;
        } else {
            S[n - 1] = finalize(wc[(n - 1) & 1], nb4, zero2, hb, 1.0f);
        }
        wc[n & 1] = nb4;
        sched_fence();
    }
    S[63] = finalize(wc[1], make_float4(0.f, 0.f, w2x0, 0.f), zero2, hb, 1.0f);
#pragma unroll
    for (int m = 0; m < 16; ++m) S[m] = stg[m * kPT];
#pragma unroll
    for (int m = 0; m < 15; ++m) S[16 + m] = stg2[m * kPT];
    lds_barrier();
    if (bot) {
        const float2* wbn = wb + (((w + 1) & 7) * 2 + hb) * 64;   // next wave's first line
#pragma unroll
        for (int n = 0; n < 64; ++n) {
            const float2 a = wbn[n];
            S[n].x -= a.x;
            S[n].y -= a.y;
        }
    }
}

// D x_K in the lane-native s layout (entry [n][t] = (d0[p], d0[p+1], d1[p], d1[p+1]) of pixel pair
// p = 4n + 2h of line r, t = 2r + h): the reverse sweep's step-K operand.  grid (128, planes) x 256.
// br: x_K in the chcat layout of several branches (grid plane q reads output plane branch_of(q).out_plane).
__global__ __launch_bounds__(256) void dx_lane_kernel(const float* __restrict__ x, float4* __restrict__ out,
                                                      Branches br) {
    const int idx = blockIdx.x * 256 + threadIdx.x;   // [n][t]
    const int n = idx >> 9, t = idx & 511;
    const int r = t >> 1, p = 4 * n + 2 * (t & 1);
    const float* xp = x + branch_of(br, blockIdx.y).out_plane * 65536;
    const float2 c = *reinterpret_cast<const float2*>(xp + r * 256 + p);
    const float2 u = *reinterpret_cast<const float2*>(xp + ((r + 255) & 255) * 256 + p);
    const float l = xp[r * 256 + ((p + 255) & 255)];
    out[(size_t)blockIdx.y * 64 * kPT + idx] = make_float4(c.x - u.x, c.y - u.y, c.x - l, c.y - c.x);
}

// grid = planes, block = 512, dynamic LDS = kLdsBytes.  K >= 1.
//   xbar    : upstream gradient of x_K (natural layout)        traj : s_1..s_{K-1}, plane256_kernel<., ., true>
//   dxK     : D x_K (dx_lane_kernel)                           sbar : lane-native sbar state (in place)
//   vsl     : lane-native Vsum accumulator                     vout : Vsum = sum_k vbar_k, natural layout
//   part    : per plane (rho_bar partial, tau_bar partial) in fp64
//   MASK    : traj is the mask-bit trajectory (plane256_kernel TRAJ 2; traj_slot in dwords); no dxK
//   br      : several branches in one grid (x_bar in the chcat layout; vout, part per grid plane)
template <bool MASK, bool WV>
__global__ __launch_bounds__(kPT) void plane256_adj_kernel(const float* __restrict__ xbar, const float* __restrict__ Cf,
                                                           const float* __restrict__ C0b,
                                                           const void* __restrict__ traj, size_t traj_slot,
                                                           const float4* __restrict__ dxK, float4* __restrict__ sbar,
                                                           float2* __restrict__ vsl, float* __restrict__ vout,
                                                           double* __restrict__ part, const float* __restrict__ prm, int K,
                                                           Branches br) {
    const BranchOf bo = branch_of(br, blockIdx.x);
    Cf += (size_t)bo.i * br.tab_f;
    C0b += (size_t)bo.i * br.tab_f;
    prm += (size_t)bo.i * br.prm_f;
    const float tau = prm[0]; const float rho = prm[1];   // device-resident scalars (setup_kernel)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2* colbuf = reinterpret_cast<float2*>(smem_raw);
    float2* tw = colbuf + kColF2;
    float2* xb = tw + kTwF2;
    float2* wb = xb + kBndF2;
    float2* sink = wb + kBndF2;
    float2* mir = sink;
    const int t = threadIdx.x;
    float* c0l = reinterpret_cast<float*>(sink + kDumF2);
    if (t < 256) c0l[t] = C0b[t];
    const bool hb = t & 1;
    const int r = t >> 1;
    const size_t plane = blockIdx.x;
    if (t < 256) {
        const int q = t >> 5, k = t & 31;
        double sn, cs;
        sincospi((double)(q * k) / 128.0, &sn, &cs);
        tw[q * kTQ + k] = make_float2((float)cs, (float)-sn);
    }
    const float2* grow = reinterpret_cast<const float2*>(xbar + bo.out_plane * 65536 + (size_t)r * 256);
    float2 S[64];
#pragma unroll
    for (int n = 0; n < 64; ++n) S[n] = grow[2 * n + hb];
    const rsrc_t cfr = make_rsrc(Cf, kTab * 4);
    const rsrc_t none = make_rsrc(Cf, 0);
    constexpr unsigned kS4 = 64 * kPT * 16, kS2 = 64 * kPT * 8;
    const float4* tb = static_cast<const float4*>(traj) + plane * 64 * kPT;
    const unsigned* mb = static_cast<const unsigned*>(traj) + plane * 16 * kPT;
    float4* sbp = sbar + plane * 64 * kPT;
    float2* vlp = vsl + plane * 64 * kPT;
    double rsum = 0.0, tsum = 0.0;
    line_forward_pair(S, hb);
    for (int k = K;; --k) {
        column_half<0, 0>(S, colbuf, tw, mir, cfr, c0l, none, nullptr, t, hb);
        column_half<0, 1>(S, colbuf, tw, mir, cfr, c0l, none, nullptr, t, hb);
        line_inverse_pair_staged(S, hb, colbuf + t, colbuf + t + 16 * kPT);
        const rsrc_t s1p = k < 2 ? none
                           : MASK ? make_rsrc(mb + (size_t)(k - 2) * traj_slot, kMaskSlotBytes)
                                  : make_rsrc(tb + (size_t)(k - 2) * traj_slot, kS4);
        // s_k / D x_K feed only rho_bar's <D vbar, D x_k>: without dxK (rho_bar not wanted) they read as 0
        const rsrc_t s2p = !dxK ? none : k == K ? make_rsrc(dxK + plane * 64 * kPT, kS4) : make_rsrc(tb + (size_t)(k - 1) * traj_slot, kS4);
        const rsrc_t sbl = k < K ? make_rsrc(sbp, kS4) : none;
        const rsrc_t sbs = k >= 2 ? make_rsrc(sbp, kS4) : none;
        // without vout (neither y_bar nor h_bar wanted) the Vsum accumulator is a zero-size resource: its
        // loads return 0 and its stores are dropped by the buffer unit, so it costs no HBM traffic
        const bool wv = WV;   // (launch_plane_adj picks WV = vout != NULL)
        const rsrc_t vlr = (k < K && wv) ? make_rsrc(vlp, kS2) : none;
        // the last step writes Vsum in the natural layout: byte r * 1024 + 16 n + 8 h
        const rsrc_t vsr = !wv ? none : k >= 2 ? make_rsrc(vlp, kS2) : make_rsrc(vout + plane * 65536, 65536 * 4);
        const unsigned vso = k >= 2 ? (unsigned)t * 8 : (unsigned)(r * 1024 + hb * 8);
        const unsigned vss = k >= 2 ? kPT * 8 : 16;
        float racc = 0.0f, tacc = 0.0f;
        row_adjoint<MASK, WV>(S, s1p, s2p, sbl, sbs, vlr, vsr, vso, vss, xb, wb, sink, colbuf, t, hb, k == K, tau, rho, racc,
                    tacc);
        rsum += racc;
        tsum += tacc;
        if (k == 1) break;
        line_forward_pair(S, hb);
    }
    // block sums in a fixed order
    for (int off = 32; off > 0; off >>= 1) {
        rsum += __shfl_down(rsum, off);
        tsum += __shfl_down(tsum, off);
    }
    double* red = reinterpret_cast<double*>(colbuf);
    lds_barrier();
    if ((t & 63) == 0) {
        red[2 * (t >> 6)] = rsum;
        red[2 * (t >> 6) + 1] = tsum;
    }
    lds_barrier();
    if (t == 0) {
        double a = 0.0, b = 0.0;
        for (int i = 0; i < kPT / 64; ++i) {
            a += red[2 * i];
            b += red[2 * i + 1];
        }
        part[2 * plane] = a;
        part[2 * plane + 1] = b;
    }
}

}  // namespace plane
}  // namespace admm
