// admm_plane_bt.hip -- isotropic TV per image plane (ADMM_ISO_PLANE): the kernels of the mode that are not a
// template variant of an existing one.  Included at the end of admm_launch.hip, behind every other kernel, so that
// the code object keeps the layout of everything in front of it.
//
// The prox is block soft-thresholding of each pixel's own 2-vector s = (s0, s1) (admm_kernels.hip bt_factor):
//   n = |s|,  f = max(1 - tau / n, 0) for n > tau, else 0,   z = f s,  u = s - f s,  w = z - u = (2f - 1) s
// It is pointwise over the two channels of one pixel, so it sits where ST sits in the anisotropic line kernels: no
// norm kernel, no factor map, no reduction over the batch.  The one change in data flow is the halo line t = T of a
// line block: its channel 0 feeds D^T, and its factor needs channel 1 too, which the anisotropic kernels never form
// there.
//   forward   line_bt_kernel (admm_kernels.hip: line_body<.., BT = true>), gen::line_upd_bt_kernel (here)
//   reverse   line_adj_bt_kernel, gen::line_adj_bt_kernel (here).  Per pixel, with wbar = rho D vbar_k, b = sbar_k,
//             a = s_{k-1}, f = f(a), n = |a| and R = sum over the 2 channels of a (2 wbar - b):
//               sbar_{k-1} = (2f - 1) wbar + (1 - f) b + [n > tau] (tau / n^3) R a
//               tau_bar   += -[n > tau] R / n
//               rho_bar   += <(2f - 1) a, D vbar_k> - <D vbar_k, D x_k>,   D x_k = s_k - (1 - f) a
//             (tests/kernel_model.py tvd_model_grads(iso=True) on one plane).  The (rho_bar, tau_bar) partial rows
//             keep the anisotropic shape: the fp64 assembly is the anisotropic one.
#include <hip/hip_runtime.h>

namespace admm {

// sbar_{k-1} of one pixel, both channels, and its (rho_bar, tau_bar) terms (added only for the block's own lines)
struct BtAdj {
    float n0, n1, rho, tau;
};
__device__ __forceinline__ BtAdj bt_adjoint(float a0, float a1, float b0, float b1, float dv0, float dv1, float tau,
                                            float rho) {
    const float n = bt_norm(a0, a1);
    const float f = bt_factor_of(n, tau);   // the forward's own f of s_{k-1}, bit for bit
    const float w0 = rho * dv0, w1 = rho * dv1;
    const float R = a0 * (2.0f * w0 - b0) + a1 * (2.0f * w1 - b1);
    const bool m = n > tau;
    const float rn = m ? __builtin_amdgcn_rcpf(n) : 0.0f;   // (n > tau >= 0: never 1 / 0)
    const float c = m ? tau * rn * rn * rn * R : 0.0f;
    const float g = (f + f) - 1.0f;
    BtAdj o;
    o.n0 = g * w0 + bt_u(b0, f) + c * a0;
    o.n1 = g * w1 + bt_u(b1, f) + c * a1;
    o.rho = g * (a0 * dv0 + a1 * dv1);
    o.tau = -R * rn;
    return o;
}

// ----------------------------------------------------------------------------------------------
// LINE_ADJ of the block-threshold prox on the 2-pass grid: line_adj_kernel's frame (natural-layout trajectory only)
// with the halo line's channel 1 of s_{k-1}, sbar_k and D vbar.
// ----------------------------------------------------------------------------------------------
template <int L, int T, bool GRP = false>
__global__ __launch_bounds__(kThreads) void line_adj_bt_kernel(const float2* __restrict__ spec1,
                                                               const float* __restrict__ sk1, const float* __restrict__ sk,
                                                               const float* __restrict__ xK,
                                                               const float* __restrict__ sb_in, float* __restrict__ sb_out,
                                                               float* __restrict__ vsum, float2* __restrict__ spec0,
                                                               double* __restrict__ part, const float2* __restrict__ twM,
                                                               int N, const float* __restrict__ prm, int first_k,
                                                               int last_k, Branches br = kOneSolve) {
    constexpr int M = 2 * L;
    constexpr int M4 = M / 4;
    constexpr int TH = T + 2;
    constexpr int P = Plan<L>::P;
    constexpr int RF = plan_radix<L, 0, true>();
    constexpr int QF = L / RF;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float2* tw = reinterpret_cast<float2*>(smem_raw);
    float2* X = tw + M;
    float2* Bf = X + TH * L;
    float2* Cf = Bf + TH * L;
    double* red = reinterpret_cast<double*>(Cf + TH * L);   // 2 doubles per wave
    const XBlk xb = xcd_block();
    const int plane = xb.y;
    const int j0 = xb.x * T;
    const size_t MN = (size_t)M * N;
    const int tid = threadIdx.x;
    const size_t poff = (size_t)plane * 2 * MN;
    const BranchOf bo = plane::plane_of<GRP>(br, plane);
    const float tau = prm[(size_t)bo.i * br.prm_f], rho = prm[(size_t)bo.i * br.prm_f + 1];   // (setup_kernel)

    for (int t = tid; t < M; t += kThreads) tw[t] = twM[t];
    load_lines<L>(spec1 + (size_t)plane * N * L, X, j0 - 1, TH, N);
    __syncthreads();
    auto uload = [&](int f, int n) { return unpack_z<L>(X + f * L, n, tw); };
    float2* Xr;
    if constexpr (P == 1) {
        Xr = Bf;
        fpass<L, L, 0, true, 2>(TH, tw, uload, LdsIO{Bf, L});
    } else if constexpr (P == 2) {
        Xr = X;
        fft_plan<L, false, true, 2>(TH, tw, Bf, Cf, L, uload, LdsIO{X, L});
    } else {
        Xr = Bf;
        plan_pass<L, 0, false, true, 2>(TH, tw, uload, LdsIO{Bf, L});
        __syncthreads();
        plan_pass<L, 1, false, true, 2>(TH, tw, LdsIO{Bf, L}, LdsIO{Cf, L});
        __syncthreads();
        plan_pass<L, 2, false, true, 2>(TH, tw, LdsIO{Cf, L}, LdsIO{Bf, L});
    }
    __syncthreads();
    const float* vb = reinterpret_cast<const float*>(Xr);       // vbar lines j0-1 .. j0+T
    float* SB0 = reinterpret_cast<float*>(Xr == X ? Bf : X);    // sbar_{k-1} ch0, lines j0..j0+T
    float* SB1 = reinterpret_cast<float*>(Cf);                  // sbar_{k-1} ch1, lines j0..j0+T-1

    float rho_acc = 0.0f, tau_acc = 0.0f;
    for (int idx = tid; idx < (T + 1) * M4; idx += kThreads) {
        const int t = idx / M4;
        const int i = (idx - t * M4) * 4;
        const size_t off = (size_t)((j0 + t) & (N - 1)) * M + i;
        const float4 vc = *reinterpret_cast<const float4*>(vb + (t + 1) * M + i);
        const float4 vp = *reinterpret_cast<const float4*>(vb + t * M + i);
        const float vl = vb[(t + 1) * M + ((i - 1) & (M - 1))];
        const float dv0[4] = {vc.x - vp.x, vc.y - vp.y, vc.z - vp.z, vc.w - vp.w};
        const float dv1[4] = {vc.x - vl, vc.y - vc.x, vc.z - vc.y, vc.w - vc.z};
        const bool own = t < T;
        float s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};   // s_{k-1}, both channels on the halo line too
        if (!first_k) load_s_quad<false>(sk1 + poff, (j0 + t) & (N - 1), i, M, MN, true, s0, s1);
        if (own) {
            // ---- rho_bar: -<Dvb, D x_k> (xK / sk null: rho_bar not wanted, no reads) ----
            float dx0[4] = {0, 0, 0, 0}, dx1[4] = {0, 0, 0, 0};
            if (last_k && xK) {
                const float* xp = xK + bo.out_plane * MN;
                const float4 xc = *reinterpret_cast<const float4*>(xp + off);
                const float4 xq = *reinterpret_cast<const float4*>(xp + (size_t)((j0 + t - 1) & (N - 1)) * M + i);
                const float xl = xp[(size_t)((j0 + t) & (N - 1)) * M + ((i - 1) & (M - 1))];
                dx0[0] = xc.x - xq.x; dx0[1] = xc.y - xq.y; dx0[2] = xc.z - xq.z; dx0[3] = xc.w - xq.w;
                dx1[0] = xc.x - xl; dx1[1] = xc.y - xc.x; dx1[2] = xc.z - xc.y; dx1[3] = xc.w - xc.z;
            } else if (!last_k && sk) {
                float a4[4], b4[4];
                load_s_quad<false>(sk + poff, (j0 + t) & (N - 1), i, M, MN, true, a4, b4);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float f = bt_factor(s0[q], s1[q], tau);
                    dx0[q] = a4[q] - bt_u(s0[q], f);
                    dx1[q] = b4[q] - bt_u(s1[q], f);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) rho_acc -= dv0[q] * dx0[q] + dv1[q] * dx1[q];
            // ---- Vsum += vbar (null: neither y_bar nor h_bar wanted) ----
            if (vsum) {
                float4* vs = reinterpret_cast<float4*>(vsum + (size_t)plane * MN + off);
                float4 acc = *vs;
                acc.x += vc.x; acc.y += vc.y; acc.z += vc.z; acc.w += vc.w;
                *vs = acc;
            }
        }
        if (!first_k) {
            float sb0[4] = {0, 0, 0, 0}, sb1[4] = {0, 0, 0, 0};   // sbar_k
            if (sb_in) {
                const float4 a = *reinterpret_cast<const float4*>(sb_in + poff + off);
                const float4 b = *reinterpret_cast<const float4*>(sb_in + poff + MN + off);
                sb0[0] = a.x; sb0[1] = a.y; sb0[2] = a.z; sb0[3] = a.w;
                sb1[0] = b.x; sb1[1] = b.y; sb1[2] = b.z; sb1[3] = b.w;
            }
            float n0[4], n1[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const BtAdj r = bt_adjoint(s0[q], s1[q], sb0[q], sb1[q], dv0[q], dv1[q], tau, rho);
                n0[q] = r.n0;
                n1[q] = r.n1;
                if (own) {
                    rho_acc += r.rho;
                    tau_acc += r.tau;
                }
            }
            *reinterpret_cast<float4*>(SB0 + t * M + i) = make_float4(n0[0], n0[1], n0[2], n0[3]);
            if (own) {
                *reinterpret_cast<float4*>(SB1 + t * M + i) = make_float4(n1[0], n1[1], n1[2], n1[3]);
                *reinterpret_cast<float4*>(sb_out + poff + off) = make_float4(n0[0], n0[1], n0[2], n0[3]);
                *reinterpret_cast<float4*>(sb_out + poff + MN + off) = make_float4(n1[0], n1[1], n1[2], n1[3]);
            }
        }
    }
    block_sum2(rho_acc, tau_acc, part + 2 * (bo.in_plane * gridDim.x + xb.x), red);
    if (first_k) return;   // k = 1: no g_0 (block-uniform)
    __syncthreads();
    // ---- g_{k-1} = D^T sbar_{k-1}, fed straight into the forward pass 0 along dim 1 ----
    float2* F0 = const_cast<float2*>(reinterpret_cast<const float2*>(vb));   // vbar dead now
    for (int idx = tid; idx < T * QF; idx += kThreads) {
        const int f = idx / QF, j = idx - f * QF;
        float2 v[RF];
#pragma unroll
        for (int r = 0; r < RF; ++r) {
            const int n = j + r * QF;
            const float2 a = *reinterpret_cast<const float2*>(SB0 + f * M + 2 * n);
            const float2 b = *reinterpret_cast<const float2*>(SB0 + (f + 1) * M + 2 * n);
            const float2 c = *reinterpret_cast<const float2*>(SB1 + f * M + 2 * n);
            const float cn = SB1[f * M + ((2 * n + 2) & (M - 1))];
            v[r].x = (a.x - b.x) + (c.x - c.y);
            v[r].y = (a.y - b.y) + (c.y - cn);
        }
        fly_core<L, RF, 0, false, 2>(v, j, tw);
        const int o = out_base<L, RF, 0>(j);
#pragma unroll
        for (int r = 0; r < RF; ++r) F0[f * L + o + r] = v[r];
    }
    __syncthreads();
    float2* Z;
    if constexpr (P == 1) {
        Z = F0;
    } else if constexpr (P == 2) {
        float2* Zb = reinterpret_cast<float2*>(SB0);
        plan_pass<L, 1, true, false, 2>(T, tw, LdsIO{F0, L}, LdsIO{Zb, L});
        __syncthreads();
        Z = Zb;
    } else {
        float2* Zb = reinterpret_cast<float2*>(SB0);
        plan_pass<L, 1, true, false, 2>(T, tw, LdsIO{F0, L}, LdsIO{Zb, L});
        __syncthreads();
        plan_pass<L, 2, true, false, 2>(T, tw, LdsIO{Zb, L}, LdsIO{F0, L});
        __syncthreads();
        Z = F0;
    }
    pack_store<L>(Z, spec0 + (size_t)plane * N * L, j0, T, N, tw);
}

namespace gen {

// line update of the block-threshold prox for T lines (line_upd_kernel's frame): s = D x + (s_old - f_old s_old),
// w = (2f - 1) s, v = rho D^T w -> half spectrum.  The halo line t = T (a ragged last block's too) forms both
// channels of s for its factor and stores neither.  s_old / s_new must not alias (halo line of s_old).
__global__ __launch_bounds__(256) void line_upd_bt_kernel(const float* __restrict__ x, const float* __restrict__ s_old,
                                                          float* __restrict__ s_new, const float* __restrict__ hty,
                                                          float2* __restrict__ spec, const float2* __restrict__ twM,
                                                          FPlan pM, int N, int Tg, const float* __restrict__ prm,
                                                          int first, Branches br = kOneSolve) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int M = pM.n, H = M / 2 + 1;
    const size_t MN = (size_t)M * N;
    float2* A = reinterpret_cast<float2*>(smem_raw);
    float2* B = A + (size_t)((Tg + 1) / 2) * M;   // P = ceil(Tg / 2) paired transforms
    float* W0 = reinterpret_cast<float*>(B + (size_t)((Tg + 1) / 2) * M);   // Tg+1 lines
    float* W1 = W0 + (size_t)(Tg + 1) * M;                       // Tg lines
    const XBlk xb = xcd_block();   // XCD-aware block order (admm_kernels.hip): neighbours share L2 lines
    const int plane = xb.y, j0 = xb.x * Tg;
    if (br.nbr == 0) prm += (size_t)plane::group_of(br, plane) * br.prm_f;   // a grouped solve: the plane's group scalars
    const float tau = prm[0]; const float rho = prm[1];   // device-resident scalars (setup_kernel)
    const int T = min(Tg, N - j0);   // the last block of a plane may be ragged (gen_nb)
    const float* xp = x + (size_t)plane * MN;
    const float* so = s_old + (size_t)plane * 2 * MN;
    float* sn = s_new + (size_t)plane * 2 * MN;
    struct UpdIn {
        float xc, xu, xl, a0, a1;
    };
    batched<kU>((T + 1) * M, [&](int idx) {
        const int t = fdiv(idx, M), i = idx - t * M;
        const int jj = wrap(j0 + t, N), jp = wrap(jj - 1, N);
        const size_t o = (size_t)jj * M + i;
        UpdIn r;
        r.xc = xp[o];
        r.xu = xp[(size_t)jp * M + i];
        r.xl = xp[(size_t)jj * M + wrap(i - 1, M)];
        r.a0 = first ? 0.0f : so[o];
        r.a1 = first ? 0.0f : so[MN + o];
        return r;
    }, [&](int idx, const UpdIn& r) {
        const int t = fdiv(idx, M), i = idx - t * M;
        const size_t o = (size_t)wrap(j0 + t, N) * M + i;
        const float fo = bt_factor(r.a0, r.a1, tau);   // (first: s_old = 0 gives f = 0, u = 0)
        const float s0 = (r.xc - r.xu) + bt_u(r.a0, fo);
        const float s1 = (r.xc - r.xl) + bt_u(r.a1, fo);
        const float f = bt_factor(s0, s1, tau);
        W0[idx] = bt_w(s0, f);
        if (t < T) {
            W1[idx] = bt_w(s1, f);
            sn[o] = s0;
            sn[MN + o] = s1;
        }
    });
    __syncthreads();
    // hty NULL: H^T y enters spectrally (column_kernel mode 16), v = rho D^T w here
    const float* hp = hty ? hty + (size_t)plane * MN + (size_t)j0 * M : nullptr;
    batched<kU>(T * M, [&](int idx) { return hp ? hp[idx] : 0.0f; }, [&](int idx, float hv) {
        const int t = fdiv(idx, M), i = idx - t * M;
        const float dtw = (W0[idx] - W0[idx + M]) + (W1[idx] - W1[t * M + wrap(i + 1, M)]);
        pack_real(A, t, i, M, fmaf(rho, dtw, hv));
    });
    pad_odd(A, T, M);
    const float2* tw = stage_tw(smem_raw, (size_t)16 * ((Tg + 1) / 2) * M + (size_t)4 * (2 * Tg + 1) * M, twM, M);
    __syncthreads();
    const float2* R = fft<false>(A, B, (T + 1) / 2, M, pM, tw);
    store_real_spectra(R, spec + ((size_t)plane * N + j0) * H, T, M);
}

// reverse step of the block-threshold prox for T lines of one plane (line_adj_kernel's frame and arguments)
__global__ __launch_bounds__(256) void line_adj_bt_kernel(const float* __restrict__ vb, const float* __restrict__ sk1,
                                                          const float* __restrict__ sk, const float* __restrict__ xK,
                                                          const float* __restrict__ sb_in, float* __restrict__ sb_out,
                                                          float* __restrict__ vsum, float2* __restrict__ spec,
                                                          double* __restrict__ part, const float2* __restrict__ twM,
                                                          FPlan pM, int N, int Tg, const float* __restrict__ prm,
                                                          Branches br = kOneSolve) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int M = pM.n, H = M / 2 + 1;
    const size_t MN = (size_t)M * N;
    float2* A = reinterpret_cast<float2*>(smem_raw);
    float2* B = A + (size_t)((Tg + 1) / 2) * M;   // P = ceil(Tg / 2) paired transforms
    float* W0 = reinterpret_cast<float*>(B + (size_t)((Tg + 1) / 2) * M);   // sbar_{k-1} ch0, Tg+1 lines
    float* W1 = W0 + (size_t)(Tg + 1) * M;                       // sbar_{k-1} ch1, Tg lines
    float* V = reinterpret_cast<float*>(smem_raw);              // vbar lines j0-1 .. j0+T (aliases A, B)
    const XBlk xb = xcd_block();   // XCD-aware block order (admm_kernels.hip): neighbours share L2 lines
    const int plane = xb.y, j0 = xb.x * Tg;
    if (br.nbr == 0) prm += (size_t)plane::group_of(br, plane) * br.prm_f;   // a grouped solve: the plane's group scalars
    const float tau = prm[0]; const float rho = prm[1];   // device-resident scalars (setup_kernel)
    const int T = min(Tg, N - j0);   // the last block of a plane may be ragged (gen_nb)
    const size_t poff = (size_t)plane * 2 * MN;
    const float* vp = vb + (size_t)plane * MN;
    batched<kU>((T + 2) * M, [&](int idx) {
        const int t = fdiv(idx, M), i = idx - t * M;
        return vp[(size_t)wrap(j0 - 1 + t, N) * M + i];
    }, [&](int idx, float v) { V[idx] = v; });
    __syncthreads();
    const float* xk = (xK && !sk) ? xK + (size_t)plane * MN : nullptr;
    const float* skp = sk ? sk + poff : nullptr;
    const float* s1p = sk1 ? sk1 + poff : nullptr;
    float racc = 0.0f, tacc = 0.0f;
    struct LAdjIn {
        float a0, a1, e0, e1, e2, vs, b0, b1;
    };
    float* vsp = vsum ? vsum + (size_t)plane * MN : nullptr;   // null: neither y_bar nor h_bar wanted
    batched<kU>((T + 1) * M, [&](int idx) {
        const int t = fdiv(idx, M), i = idx - t * M;
        const int j = wrap(j0 + t, N);
        const size_t o = (size_t)j * M + i;
        const bool own = t < T;
        LAdjIn r;
        r.a0 = s1p ? s1p[o] : 0.0f;
        r.a1 = s1p ? s1p[MN + o] : 0.0f;
        r.e0 = r.e1 = r.e2 = r.vs = 0.0f;
        if (own) {   // D x_k operands: x_K and its two neighbours, or s_k
            if (xk) {
                r.e0 = xk[o];
                r.e1 = xk[(size_t)wrap(j - 1, N) * M + i];
                r.e2 = xk[(size_t)j * M + wrap(i - 1, M)];
            } else {
                r.e0 = skp[o];
                r.e1 = skp[MN + o];
            }
            r.vs = vsp ? vsp[o] : 0.0f;
        }
        r.b0 = (s1p && sb_in) ? sb_in[poff + o] : 0.0f;
        r.b1 = (s1p && sb_in) ? sb_in[poff + MN + o] : 0.0f;
        return r;
    }, [&](int idx, const LAdjIn& r) {
        const int t = fdiv(idx, M), i = idx - t * M;
        const size_t o = (size_t)wrap(j0 + t, N) * M + i;
        const bool own = t < T;
        const float vc = V[(t + 1) * M + i];
        const float dv0 = vc - V[t * M + i];
        const float dv1 = vc - V[(t + 1) * M + wrap(i - 1, M)];
        if (own) {
            float d0, d1;
            if (xk) {
                d0 = r.e0 - r.e1;
                d1 = r.e0 - r.e2;
            } else {
                const float f = bt_factor(r.a0, r.a1, tau);   // (k = 1: s_0 = 0 gives u = 0)
                d0 = r.e0 - bt_u(r.a0, f);
                d1 = r.e1 - bt_u(r.a1, f);
            }
            racc -= dv0 * d0 + dv1 * d1;
            if (vsp) vsp[o] = r.vs + vc;
        }
        if (!s1p) return;   // k = 1: no sbar_0 (block-uniform)
        const BtAdj q = bt_adjoint(r.a0, r.a1, r.b0, r.b1, dv0, dv1, tau, rho);
        W0[idx] = q.n0;
        if (own) {
            W1[idx] = q.n1;
            racc += q.rho;
            tacc += q.tau;
            sb_out[poff + o] = q.n0;
            sb_out[poff + MN + o] = q.n1;
        }
    });
    block_pair(racc, tacc, part + 2 * ((size_t)plane * gridDim.x + xb.x));
    if (!s1p) return;
    __syncthreads();   // W0/W1 complete; V (aliasing A, B) is dead
    for (int idx = threadIdx.x; idx < T * M; idx += blockDim.x) {
        const int t = fdiv(idx, M), i = idx - t * M;
        const float g = (W0[idx] - W0[idx + M]) + (W1[idx] - W1[t * M + wrap(i + 1, M)]);
        pack_real(A, t, i, M, g);
    }
    pad_odd(A, T, M);
    const float2* tw = stage_tw(smem_raw, (size_t)16 * ((Tg + 1) / 2) * M + (size_t)4 * (2 * Tg + 1) * M, twM, M);
    __syncthreads();
    const float2* R = fft<false>(A, B, (T + 1) / 2, M, pM, tw);
    store_real_spectra(R, spec + ((size_t)plane * N + j0) * H, T, M);
}

}  // namespace gen
}  // namespace admm
