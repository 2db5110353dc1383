// admm_launch.hip -- launch sequencing of the ADMM solve (see capi_internal.hpp), enqueued on the caller's stream
// exactly as plan_paths (admm_paths.hip) decided.  Reference: /root/reference/src/ops/ops.jl:99-188.
//   template dispatch    the instantiation list of the 2-pass kernels (its order is the code object's layout)
//   workspace views      a Layout / BwdLayout / MultiLayout resolved into typed pointers once
//   shared steps         the natural-layout isotropic norm, the s slots of an iteration, the spectral convolution
//   TwoPass              one 2-pass grid -- a single or grouped solve, or several branches in one grid -- and the
//                        two sequences every caller runs on it:
//     two_pass_forward   PREP (Y_h = F(H^T y): line transform, column x conj(Sigma_c), ops.jl:71-81), K x COLUMN,
//                        (K-1) x LINE (or ISO_A, norm, ISO_B), 1 x FINAL                        (ops.jl:166-174)
//     two_pass_reverse   line transform of x_bar, then per step COLUMN and the line adjoint (or ISO_ADJ_A, _R, _B)
//   run_forward          a Call's planes (all, or one chunk): SETUP (twiddles + C, ops.jl:22-37; a grouped call's per
//                        group), then the fused / CU-resident / 2-pass path
//   run_forward_generic  the runtime-length path (its own kernels: a separate inverse, the smooth-length alternatives)
//   launch_backward      the one adjoint driver of single and grouped calls: recording forward, one reverse sweep (fused,
//                        fused isotropic, runtime-length, 2-pass), assembly; grouping enters through Grouping only
//   launch_*_multi       the one-grid multi-branch solve: the fused kernels, or the same TwoPass sequences
//   launch_forward_state the resumable solve: the forward from s_0 (state_start: v_0 in place of the cleared first line
//                        spectrum) or from the zero state, then the end kernels (s_K, residual norms; state_kernels.hip)
// A call of any family arrives as the Call / Grads descriptors of capi_internal.hpp, never as a positional parameter
// list, with the plan (PathPlan, or the layout planned for it) that plan_paths made of it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "capi_internal.hpp"
#include "admm_kernels.hip"
#include "admm_generic.hip"
#include "admm_backward.hip"
#include "admm_generic_bwd.hip"
#include "smooth_api.hpp"
#include "resident_api.hpp"
#include "state_api.hpp"

namespace admm_capi {

using namespace admm;

// ---- template dispatch -----------------------------------------------------------------------
// This translation unit alone compiles the 2-pass kernels, and they land in the code object in the order in which
// the host code first names them: these dispatchers (and launch_line_adj / launch_iso_adj_a / launch_iso_adj_b
// further down) are that instantiation list.  Their order fixes the code object's layout, and code placement
// alone is measurable (0.8 % at c2): keep them where they are and in this order.

template <typename K>
void set_lds(K kernel, size_t lds) {
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// (L, T) pairs that line_T() can return
#define ADMM_LT_CASES(X)                                                                           \
    X(2, 2) X(2, 4) X(2, 8) X(2, 16) X(4, 2) X(4, 4) X(4, 8) X(4, 16) X(8, 2) X(8, 4) X(8, 8) X(8, 16) \
    X(16, 2) X(16, 4) X(16, 8) X(16, 16) X(32, 2) X(32, 4) X(32, 8) X(32, 16) X(64, 2) X(64, 4)      \
    X(64, 8) X(64, 16) X(128, 2) X(128, 4) X(128, 8) X(128, 16) X(256, 2) X(256, 4) X(256, 8)       \
    X(512, 2) X(512, 4)
#define ADMM_N_CASES(X) X(2) X(4) X(8) X(16) X(32) X(64) X(128) X(256) X(512) X(1024)

// br / map (several branches in one grid): the line transforms read / write the shared input plane or the chcat
// plane of each grid plane (admm_kernels.hip PlaneMap)
int launch_line_fwd(int L, int T, dim3 g, size_t lds, hipStream_t s, const float* src, float2* spec,
                    const float2* twM, int N, const Branches& br = kOneSolve, int map = kMapGrid) {
#define X(l, t)                                                                     \
    if (L == l && T == t) {                                                         \
        set_lds(line_fwd_kernel<l, t>, lds);                                        \
        line_fwd_kernel<l, t><<<g, kThreads, lds, s>>>(src, spec, twM, N, br, map); \
        return 0;                                                                   \
    }
    ADMM_LT_CASES(X)
#undef X
    return -1;
}

int launch_line_inv(int L, int T, dim3 g, size_t lds, hipStream_t s, const float2* spec, float* dst,
                    const float2* twM, int N, const Branches& br = kOneSolve, int map = kMapGrid) {
#define X(l, t)                                                                     \
    if (L == l && T == t) {                                                         \
        set_lds(line_inv_kernel<l, t>, lds);                                        \
        line_inv_kernel<l, t><<<g, kThreads, lds, s>>>(spec, dst, twM, N, br, map); \
        return 0;                                                                   \
    }
    ADMM_LT_CASES(X)
#undef X
    return -1;
}

int launch_line(int L, int T, dim3 g, size_t lds, hipStream_t s, const float2* spec1, float2* spec0,
                const float* so, float* sn, const float* hty, const float2* twM, int N, const float* prm,
                int sz, int nt = kThreads, const Branches& br = kOneSolve) {
    if (br.nbr == 0) {   // a grouped solve: the GRP instantiations (group scalars per plane)
#define X3(l, t, n)                                                                                       \
        if (L == l && T == t && nt == n) {                                                                \
            set_lds(line_kernel<l, t, n, true>, lds);                                                     \
            line_kernel<l, t, n, true><<<g, n, lds, s>>>(spec1, spec0, so, sn, hty, twM, N, prm, sz, br); \
            return 0;                                                                                     \
        }
#define X(l, t) X3(l, t, kThreads)
        X3(256, 8, 512) X3(256, 16, 1024) X3(256, 4, 512) X3(256, 8, 1024)
        ADMM_LT_CASES(X)
#undef X
#undef X3
        return -1;
    }
    if (nt != kThreads) {   // wider blocks at 512-point lines (update kernel, line_T_upd)
#define X(l, t, n)                                                                                       \
        if (L == l && T == t && nt == n) {                                                               \
            set_lds(line_kernel<l, t, n>, lds);                                                          \
            line_kernel<l, t, n><<<g, n, lds, s>>>(spec1, spec0, so, sn, hty, twM, N, prm, sz, br);     \
            return 0;                                                                                    \
        }
        X(256, 8, 512) X(256, 16, 1024) X(256, 4, 512) X(256, 8, 1024)
#undef X
        return -1;
    }
#define X(l, t)                                                                                          \
    if (L == l && T == t) {                                                                              \
        set_lds(line_kernel<l, t>, lds);                                                                 \
        line_kernel<l, t><<<g, kThreads, lds, s>>>(spec1, spec0, so, sn, hty, twM, N, prm, sz, br); \
        return 0;                                                                                        \
    }
    ADMM_LT_CASES(X)
#undef X
    return -1;
}

// planes: per branch; ngb: plane groups per branch (grid y = branches x ngb), 0: one branch
int launch_iso_a(int L, int T, dim3 g, size_t lds, hipStream_t s, const float2* spec1, const float* so, float* sn,
                 const float* fmap, float* part, const float2* twM, int N, int planes, int G, int sz, int ngb = 0) {
#define X(l, t)                                                                                             \
    if (L == l && T == t) {                                                                                 \
        set_lds(iso_a_kernel<l, t>, lds);                                                                   \
        iso_a_kernel<l, t><<<g, kThreads, lds, s>>>(spec1, so, sn, fmap, part, twM, N, planes, G, sz, ngb); \
        return 0;                                                                                           \
    }
    ADMM_LT_CASES(X)
#undef X
    return -1;
}

int launch_iso_b(int L, int T, dim3 g, size_t lds, hipStream_t s, const float* sn, const float* fmap,
                 const float* hty, float2* spec0, const float2* twM, int N, const float* prm,
                 const Branches& br = kOneSolve) {
#define X(l, t)                                                                               \
    if (L == l && T == t) {                                                                   \
        set_lds(iso_b_kernel<l, t>, lds);                                                     \
        iso_b_kernel<l, t><<<g, kThreads, lds, s>>>(sn, fmap, hty, spec0, twM, N, prm, br);  \
        return 0;                                                                             \
    }
    ADMM_LT_CASES(X)
#undef X
    return -1;
}

template <int MUL, bool SAVE, bool ACCQ, int YH = YH_NONE, bool GRP = false>
int launch_column_t(int N, dim3 g, size_t lds, hipStream_t s, const float2* src, float2* dst, const float* C,
                    const float2* G, const float2* twN, int L, int KB, float cs, float2* vsave, double* Qp,
                    const Branches& br, float2* yh = nullptr) {
    const int nt = column_threads(N);
#define X(v)                                                                                                   \
    if (N == v && nt == kThreads) {                                                                            \
        set_lds(column_kernel<v, MUL, SAVE, ACCQ, kThreads, YH, GRP>, lds);                                         \
        column_kernel<v, MUL, SAVE, ACCQ, kThreads, YH, GRP><<<g, kThreads, lds, s>>>(src, dst, C, G, twN, L, KB, cs,  \
                                                                                  vsave, Qp, br, yh);             \
        return 0;                                                                                              \
    }
    ADMM_N_CASES(X)
#undef X
#define X(v)                                                                                                   \
    if (N == v && nt == 512) {                                                                                 \
        set_lds(column_kernel<v, MUL, SAVE, ACCQ, 512, YH, GRP>, lds);                                              \
        column_kernel<v, MUL, SAVE, ACCQ, 512, YH, GRP><<<g, 512, lds, s>>>(src, dst, C, G, twN, L, KB, cs, vsave, Qp, br, \
                                                                       yh);                                        \
        return 0;                                                                                              \
    }
    X(256) X(512) X(1024)
#undef X
#define X(v)                                                                                                   \
    if (N == v && nt == 1024) {                                                                                \
        set_lds(column_kernel<v, MUL, SAVE, ACCQ, 1024, YH, GRP>, lds);                                             \
        column_kernel<v, MUL, SAVE, ACCQ, 1024, YH, GRP><<<g, 1024, lds, s>>>(src, dst, C, G, twN, L, KB, cs, vsave, Qp,  \
                                                                         br, yh);                                   \
        return 0;                                                                                              \
    }
    X(256) X(512) X(1024)
#undef X
    return -1;
}

// The grouped adjoint's GRP instantiations (modes 0, 2, 4, 7 and the line adjoint) are named at the end of this file,
// so that they land behind every existing kernel in the code object.
int launch_column_grouped_adj(int N, int mode, dim3 g, size_t lds, hipStream_t s, const float2* src, float2* dst,
                              const float* C, const float2* G, const float2* twN, int L, int KB, float cs, float2* vsave,
                              double* Qp, const Branches& br, float2* yh);
int launch_line_adj_grouped(int L, int T, dim3 g, size_t lds, hipStream_t s, const float2* spec1, const float* sk1,
                            const float* sk, const float* xK, const float* sb_in, float* sb_out, float* vsum, float2* spec0,
                            double* part, const float2* twM, int N, const float* prm, int first_k, int last_k, bool ln,
                            const Branches& br);

// The per-plane isotropic mode's kernels (ADMM_ISO_PLANE: line_bt_kernel and admm_plane_bt.hip) are named at the end
// of this file too.  The 2-pass launchers take launch_line's / launch_line_adj's arguments, the runtime-length ones the
// kernels' own.
int launch_line_bt(int L, int T, dim3 g, size_t lds, hipStream_t s, const float2* spec1, float2* spec0, const float* so,
                   float* sn, const float2* twM, int N, const float* prm, int sz, int nt, const Branches& br);
int launch_line_adj_bt(int L, int T, dim3 g, size_t lds, hipStream_t s, const float2* spec1, const float* sk1,
                       const float* sk, const float* xK, const float* sb_in, float* sb_out, float* vsum, float2* spec0,
                       double* part, const float2* twM, int N, const float* prm, int first_k, int last_k,
                       const Branches& br);
int launch_gen_line_upd_bt(dim3 g, size_t lds, hipStream_t s, const float* x, const float* so, float* sn, float2* spec,
                           const float2* twM, const admm::gen::FPlan& pM, int N, int T, const float* prm, int first,
                           const Branches& br);
int launch_gen_line_adj_bt(dim3 g, size_t lds, hipStream_t s, const float* vb, const float* sk1, const float* sk,
                           const float* xK, const float* sb_in, float* sb_out, float* vsum, float2* spec, double* part,
                           const float2* twM, const admm::gen::FPlan& pM, int N, int T, const float* prm,
                           const Branches& br);

// mode: 0 = x-update C, 1 = conj(Sigma_c) (H^T), 2 = Sigma_c (H), 3 = C + save spectrum, 4 = C + accumulate Q;
// 5 = Y_h = cs conj(Sigma_c) F y stored to yh (G NULL: Y_h = cs F y), no inverse; 6 = + yh, x C; 7 = + yh, save, x C
// (admm_kernels.hip YH_STORE / YH_ADD: H^T y in the spectral domain); br: several branches (C per branch, br.tab_f
// floats apart)
int launch_column(int N, int mode, dim3 g, size_t lds, hipStream_t s, const float2* src, float2* dst,
                  const float* C, const float2* G, const float2* twN, int L, int KB, float cs,
                  float2* vsave = nullptr, double* Qp = nullptr, const Branches& br = kOneSolve, float2* yh = nullptr) {
    if (br.nbr == 0) {   // a grouped solve: Y_h prep and the x-update; the recording's and the sweep's modes below
        if (mode == 5) return launch_column_t<1, false, false, YH_STORE, true>(N, g, lds, s, src, dst, C, G, twN, L, KB, cs, vsave, Qp, br, yh);
        if (mode == 6) return launch_column_t<0, false, false, YH_ADD, true>(N, g, lds, s, src, dst, C, G, twN, L, KB, cs, vsave, Qp, br, yh);
        return launch_column_grouped_adj(N, mode, g, lds, s, src, dst, C, G, twN, L, KB, cs, vsave, Qp, br, yh);
    }
    switch (mode) {
        case 5: return launch_column_t<1, false, false, YH_STORE>(N, g, lds, s, src, dst, C, G, twN, L, KB, cs, vsave, Qp, br, yh);
        case 6: return launch_column_t<0, false, false, YH_ADD>(N, g, lds, s, src, dst, C, G, twN, L, KB, cs, vsave, Qp, br, yh);
        case 7: return launch_column_t<0, true, false, YH_ADD>(N, g, lds, s, src, dst, C, G, twN, L, KB, cs, vsave, Qp, br, yh);
        case 0: return launch_column_t<0, false, false>(N, g, lds, s, src, dst, C, G, twN, L, KB, cs, vsave, Qp, br);
        case 1: return launch_column_t<1, false, false>(N, g, lds, s, src, dst, C, G, twN, L, KB, cs, vsave, Qp, br);
        case 2: return launch_column_t<2, false, false>(N, g, lds, s, src, dst, C, G, twN, L, KB, cs, vsave, Qp, br);
        case 3: return launch_column_t<0, true, false>(N, g, lds, s, src, dst, C, G, twN, L, KB, cs, vsave, Qp, br);
        case 4: return launch_column_t<0, false, true>(N, g, lds, s, src, dst, C, G, twN, L, KB, cs, vsave, Qp, br);
    }
    return -1;
}

// ---- generic-size path (admm_generic.hip) ----------------------------------------------------
admm::gen::FPlan make_fplan(int n) {
    admm::gen::FPlan p{};
    p.n = n;
    int m = n;
    auto add = [&](int r) { p.r[p.nf++] = r; m /= r; };
    while (m % 8 == 0) add(8);
    if (m % 4 == 0) add(4);
    if (m % 2 == 0) add(2);
    while (m % 3 == 0) add(3);
    while (m % 5 == 0) add(5);
    for (int f = 7; f * f <= m; f += 2)
        while (m % f == 0) add(f);
    if (m > 1) add(m);
    return p;
}

// the caller's cross-shard sum of an M x N map (isotropic prox over a sharded batch)
int call_reducer(const admm_batch_reducer* red, float* buf, size_t count, hipStream_t s) {
    const int r = red->fn(buf, count, reinterpret_cast<void*>(s), red->user);
    if (r != 0) return fail(ADMM_E_REDUCER, "batch reducer returned %d", r);
    return ADMM_OK;
}

// ---- workspace views: a layout's offsets resolved into typed pointers once ----------------------------------
template <typename T>
T* at(unsigned char* ws, size_t off) {
    return reinterpret_cast<T*>(ws + off);
}

struct FwdView {
    float2 *twM, *twN;
    float* C;
    float2* G;     // null without a PSF
    float* prm;    // tau = lambda / rho (ops.jl:20), rho, lambda
    float* hty;    // H^T y -- or, on the 2-pass and runtime-length paths, Y_h = F(H^T y) (float2, see yh())
    float* s[2];
    float2 *spec0, *spec1;
    float *fmap, *part, *xg;   // isotropic f map and plane-group partials; runtime-length x
    void* F;                   // lane-native tables (256 x 256)
    float2* yh() const { return reinterpret_cast<float2*>(hty); }
};
FwdView view(unsigned char* ws, const Layout& l, bool psf) {
    return FwdView{at<float2>(ws, l.twM), at<float2>(ws, l.twN), at<float>(ws, l.C), psf ? at<float2>(ws, l.G) : nullptr,
                   at<float>(ws, l.prm), at<float>(ws, l.hty), {at<float>(ws, l.sA), at<float>(ws, l.sB)},
                   at<float2>(ws, l.spec0), at<float2>(ws, l.spec1), at<float>(ws, l.fmap), at<float>(ws, l.part),
                   at<float>(ws, l.xg), ws + l.F};
}

// what a reverse sweep reads and writes besides the forward view's tables and spectra
struct SweepBufs {
    const float* traj;   // s_k slots (natural layout; the 2-pass line adjoint also reads the fused kernel's)
    const float* nrm;    // |s_k| slots (isotropic)
    float2* v;           // h_bar: the recorded dim-2 spectra and the planes' Q accumulators, else both null
    double* Qp;
    float* sb[2];        // sbar ping-pong
    float* vsum;         // Vsum = sum_k vbar_k (null: neither y_bar nor h_bar wanted)
    float *wbar, *Rmap, *Rpart;   // isotropic
    double* part;        // (rho_bar, tau_bar) partial rows
    const float* xK;     // the forward's output: enters rho_bar only (null without it)
};

struct BwdView {
    FwdView f;
    SweepBufs b;
    double2* sig;
    double *Q, *hpart, *hcorr, *hA, *rt, *rtmp;
};
BwdView view(unsigned char* ws, const BwdLayout& l, bool psf, bool iso, bool want_h, bool want_v, const float* xK) {
    BwdView v{view(ws, l.f, psf)};
    v.b = SweepBufs{at<float>(ws, l.traj_s), iso ? at<float>(ws, l.traj_n) : nullptr,
                    want_h ? at<float2>(ws, l.traj_v) : nullptr, want_h ? at<double>(ws, l.Qp) : nullptr,
                    {at<float>(ws, l.sbA), at<float>(ws, l.sbB)}, want_v ? at<float>(ws, l.vsum) : nullptr,
                    iso ? at<float>(ws, l.wbar) : nullptr, iso ? at<float>(ws, l.Rmap) : nullptr,
                    iso ? at<float>(ws, l.Rpart) : nullptr, at<double>(ws, l.rpart), xK};
    v.sig = want_h ? at<double2>(ws, l.sig) : nullptr;
    v.Q = at<double>(ws, l.Q);
    v.hpart = at<double>(ws, l.hpart);
    v.hcorr = psf ? at<double>(ws, l.hcorr) : nullptr;
    v.hA = want_h ? at<double>(ws, l.hA) : nullptr;
    v.rt = at<double>(ws, l.rt);
    v.rtmp = at<double>(ws, l.rtmp);
    return v;
}

// the one-grid call's slots that both of its grids (fused, 2-pass) use
struct MultiView {
    float* prm;
    float2 *twM, *twN;
    float2* hln;          // fused: lane-native H^T y, then each branch's Vsum; 2-pass: Y_h
    unsigned char *sln, *traj, *sbar, *vsl;
    float *fmap, *qpart, *nrm, *rmap;
    double *part, *rt, *rtmp;
};
MultiView view(unsigned char* ws, const MultiLayout& l) {
    return MultiView{at<float>(ws, l.prm), at<float2>(ws, l.twM), at<float2>(ws, l.twN), at<float2>(ws, l.hln),
                     ws + l.sln, ws + l.traj, ws + l.sbar, ws + l.vsl, at<float>(ws, l.fmap), at<float>(ws, l.qpart),
                     at<float>(ws, l.nrm), at<float>(ws, l.rmap), at<double>(ws, l.part), at<double>(ws, l.rt),
                     at<double>(ws, l.rtmp)};
}

// ---- shared steps ---------------------------------------------------------------------------------------------
// Natural-layout isotropic batch norm: the plane groups' (or planes') |s|^2 partials -> BT factor f (and |s| when
// recording).  A sharded batch splits it into the shard sum, the caller's all-reduce of the M x N map and the factor.
// ny branches (grid y), each with its own partials, maps and {tau, rho, lambda} block prm_f floats apart.
int iso_norm_step(Launcher& ln, const float* part, float* fmap, int ngroups, size_t MN, const float* prm, float* nrm_out,
                  const admm_batch_reducer* red, unsigned ny = 1, unsigned prm_f = 0) {
    hipStream_t s = ln.s;
    const int nb = (int)((MN + 63) / 64);   // 64 pixels per block (group_sum)
    const dim3 gr(nb < 2048 ? nb : 2048, ny);
    if (!red)
        return ln.run(ADMM_K_NORM, [&] {
            hipLaunchKernelGGL(admm::iso_r_kernel, gr, dim3(kThreads), 0, s, part, fmap, ngroups, MN, prm, nrm_out, prm_f);
        });
    int rc = ln.run(ADMM_K_NORM, [&] {
        hipLaunchKernelGGL(admm::iso_sum_kernel, gr, dim3(kThreads), 0, s, part, fmap, ngroups, MN);
    });
    if (rc) return rc;
    rc = call_reducer(red, fmap, MN, s);
    if (rc) return rc;
    return ln.run(ADMM_K_NORM, [&] {
        hipLaunchKernelGGL(admm::iso_fin_kernel, gr, dim3(kThreads), 0, s, fmap, MN, prm, nrm_out);
    });
}

// A state call's warm start: v_0 = rho D^T (z_0 - u_0) of the caller's s_0 into st.v0 -- isotropic: the batch norm of
// s_0 first, its factor map left in fmap for iteration 1.  The caller line-transforms v_0 into the first line spectrum
// (a cold call transforms zeros), and iteration 1 then reads s_0 as s_old with the kernels' s_zero / first flag off.
int state_start(Launcher& ln, const StateIO& st, bool iso, int M, int N, size_t planes, float* part, float* fmap,
                const float* prm) {
    hipStream_t s = ln.s;
    const size_t MN = (size_t)M * N;
    if (iso) {
        const int ng = iso_ngroups(planes);
        int rc = ln.run(ADMM_K_NORM, [&] { return admm::st::launch_sq(st.in, part, MN, planes, iso_group(planes), ng, s); });
        if (rc) return rc;
        rc = iso_norm_step(ln, part, fmap, ng, MN, prm, nullptr, nullptr);
        if (rc) return rc;
    }
    return ln.run(ADMM_K_PREP, [&] { return admm::st::launch_v0(st.in, iso ? fmap : nullptr, st.v0, M, N, planes, prm, s); });
}

// Iteration it = 1 .. K-1 reads s_{it-1} and writes s_it: a recording keeps s_it in trajectory slot it - 1; without
// one the two buffers take turns (isotropic: b1 = b0, s is updated in place).  Iteration 1 reads no s (the kernels'
// s_zero / first flag): so is then sn itself, any valid pointer would do.
struct Slots {
    const float* so;
    float* sn;
};
Slots fwd_slots(int it, float* traj, size_t sstride, float* b0, float* b1) {
    float* sn = traj ? traj + (size_t)(it - 1) * sstride : (it & 1) ? b0 : b1;
    if (it == 1) return {sn, sn};
    return {traj ? traj + (size_t)(it - 2) * sstride : (it & 1) ? b1 : b0, sn};
}

// ---- one 2-pass grid ------------------------------------------------------------------------------------------
// Grid plane q of several branches in one grid is branch i's solve of input plane loc (q = i ppb + loc; y shared,
// x_out / x_bar in the chcat layout: the first and last line transform map planes, admm_kernels.hip PlaneMap); per
// branch its C table, {tau, rho, lambda}, f map, |s| slots, R map, plane groups and partial rows.
struct TwoPass {
    Launcher& ln;
    int M, N, L, T, KB;
    int Tu, nTu;               // the update kernel's lines and threads per block (512-point lines)
    size_t planes, MN;
    dim3 gl, gc, gu;           // line transforms and adjoints, column pass, line update
    size_t flds, clds, llds;
    const float2 *twM, *twN;
    const float* C;
    const float2* G;
    const float* prm;
    float2 *spec0, *spec1, *yh;
    Branches br;               // column pass and line update: one solve, a grouped solve, or the branches
    Branches bro;              // every other kernel: one solve (a grouped solve too), or the branches
    int map_in, map_out;       // plane maps of the first / last line transform
    // isotropic: ng plane groups in all (ISO_A's grid y) of Gp planes, ngb per branch (ngb_k: the kernels' argument,
    // 0 for one solve), gplanes planes per branch; the norm kernels' grid y and prm stride; floats per |s| slot
    float *fmap, *qpart;
    int ng, Gp, ngb, ngb_k, gplanes;
    unsigned ny, prm_f;
    size_t nstride;
    // reverse sweep: partial rows per step, doubles between the branches' row blocks, ISO_ADJ_R's first row of a step
    int rows;
    size_t pbs;
    int r_off;
    // ADMM_ISO_PLANE: the anisotropic sequences with the block-threshold line update / line adjoint
    bool bt = false;
};

TwoPass two_pass_grid(Launcher& ln, int M, int N, size_t planes, int T) {
    TwoPass c{ln, M, N, M / 2, T, column_KB(M, N)};
    // the per-iteration line update runs 4-line blocks at 512-point lines (its just-in-time loads let 4 of
    // them share a CU, admm_kernels.hip line_kernel); the one-off line transforms keep T
    // 512-point lines: 8-line update blocks of 512 threads (round 5, tools/c4_line_sweep.sh: line pass 1.217 ->
    // 1.196 ms at c4; 4 lines x 256 threads was round 1's choice; 16 x 1024, 4 x 512 and 8 x 1024 slower:
    // profiles/r05_c4_line_sweep.jsonl)
    c.Tu = (M == 512 && T > 4) ? 8 : T;
    c.nTu = (M == 512 && c.Tu == 8) ? 512 : kThreads;
    c.planes = planes;
    c.MN = (size_t)M * N;
    c.gl = dim3(N / T, (unsigned)planes);
    c.gc = dim3(c.L / c.KB, (unsigned)planes);
    c.gu = dim3(N / c.Tu, (unsigned)planes);
    c.flds = fwdinv_lds(M, T);
    c.clds = column_lds(N, c.KB);
    c.llds = line_lds(M, c.Tu);
    return c;
}

// a single solve, or (grp) a grouped one: the descriptor of its C / G tables, tab_f apart, and scalar blocks
TwoPass two_pass_single(Launcher& ln, int M, int N, size_t planes, int T, const FwdView& v, const Branches& grp = kOneSolve) {
    TwoPass c = two_pass_grid(ln, M, N, planes, T);
    c.twM = v.twM, c.twN = v.twN, c.C = v.C, c.G = v.G, c.prm = v.prm;
    c.spec0 = v.spec0, c.spec1 = v.spec1, c.yh = v.yh();   // the workspace's H^T y slot holds Y_h on this path
    c.br = grp, c.bro = kOneSolve;
    c.map_in = c.map_out = kMapGrid;
    c.fmap = v.fmap, c.qpart = v.part;
    c.ng = c.ngb = iso_ngroups(planes), c.Gp = iso_group(planes), c.ngb_k = 0, c.gplanes = (int)planes;
    c.ny = 1, c.prm_f = 0, c.nstride = c.MN;
    return c;
}

// ---- several branches in one grid: the kernels' descriptor over the fused grid's lane-native tables or the 2-pass
// grid's C tables, and the 2-pass grid over every branch's planes ----
Branches multi_branches(const Call& m, size_t table_bytes) {
    return Branches{m.P * m.B, m.nbranch, m.P, (unsigned)(table_bytes / 4), 4u};
}

TwoPass two_pass_multi(Launcher& ln, const Call& m, int T, const MultiLayout& Ly) {
    unsigned char* ws = static_cast<unsigned char*>(m.workspace);
    const int nbr = m.nbranch;
    TwoPass c = two_pass_grid(ln, kMultiM, kMultiN, m.grid_planes(), T);
    const MultiView v = view(ws, Ly);
    c.twM = v.twM, c.twN = v.twN, c.C = at<float>(ws, Ly.C), c.G = nullptr, c.prm = v.prm;
    // H^T y = y (no PSF) in the spectral domain: Y_h = F y per grid plane in the hln slot, unused by the 2-pass grid
    c.spec0 = at<float2>(ws, Ly.spec0), c.spec1 = at<float2>(ws, Ly.spec1), c.yh = v.hln;
    c.br = c.bro = multi_branches(m, multi_C_bytes());
    c.map_in = kMapIn, c.map_out = kMapOut;
    c.fmap = v.fmap, c.qpart = v.qpart;
    c.ng = nbr * Ly.ngb, c.Gp = Ly.G, c.ngb = c.ngb_k = Ly.ngb, c.gplanes = m.P * m.B;
    c.ny = (unsigned)nbr, c.prm_f = 4u, c.nstride = (size_t)nbr * c.MN;
    c.rows = Ly.rows_b, c.pbs = Ly.pbs, c.r_off = Ly.nblk_a;
    return c;
}

// dst = F^-1 [multiplier] F src, spectrally (mode 1: conj(Sigma_c), H^T; 2: Sigma_c, H; launch_column); br: a
// grouped solve's descriptor (mode 2: every plane with its group's G table)
int two_pass_conv(const TwoPass& c, int cls, int mode, const float* src, float* dst, const Branches& br = kOneSolve) {
    Launcher& ln = c.ln;
    hipStream_t s = ln.s;
    int rc = ln.run(cls, [&] { return launch_line_fwd(c.L, c.T, c.gl, c.flds, s, src, c.spec0, c.twM, c.N); });
    if (rc) return rc;
    rc = ln.run(cls, [&] {
        return launch_column(c.N, mode, c.gc, c.clds, s, c.spec0, c.spec1, c.C, c.G, c.twN, c.L, c.KB, 1.0f, nullptr,
                             nullptr, br);
    });
    if (rc) return rc;
    return ln.run(cls, [&] { return launch_line_inv(c.L, c.T, c.gl, c.flds, s, c.spec1, dst, c.twM, c.N); });
}

// PREP: Y_h = F(H^T y) = conj(Sigma_c) F y as a 2-D packed spectrum straight from F y (line transform, column
// transform x conj(Sigma_c)), never H^T y in space: every iteration adds it to the spectrum of rho D^T w in
// the column pass, so the per-iteration fp32 transforms carry only rho D^T w (x 16x, y_bar / h_bar ~2-9x closer
// to the fp64 oracle than with H^T y added before the line transform; DESIGN.md s1 "H^T y in the spectrum").
// Iteration 1 (w = 0) transforms a zero line spectrum and adds Y_h.  Then K x column, (K-1) x line update (isotropic:
// ISO_A over the plane groups, the batch norm, ISO_B) and the final inverse.
// tr: s_it into trajectory slot it - 1, the dim-2 spectrum of iteration it (before the multiply, h_bar) into slot
// it - 1 of tr.v, |s_it| into norm slot it - 1; b0 / b1: the s buffers without a recording (fwd_slots).
// st (a state call) with st->in: the first line spectrum is that of v_0 (state_start) and iteration 1 reads s_0.
int two_pass_forward(const TwoPass& c, const float* y, float* x_out, int maxit, bool iso, const Traj& tr, float* b0,
                     float* b1, const admm_batch_reducer* red = nullptr, const StateIO* st = nullptr) {
    const float* s0 = st ? st->in : nullptr;
    Launcher& ln = c.ln;
    hipStream_t s = ln.s;
    int rc = ln.run(ADMM_K_PREP, [&] {
        return launch_line_fwd(c.L, c.T, c.gl, c.flds, s, y, c.spec0, c.twM, c.N, c.bro, c.map_in);
    });
    if (rc) return rc;
    rc = ln.run(ADMM_K_PREP, [&] {
        return launch_column(c.N, 5, c.gc, c.clds, s, c.spec0, c.spec1, c.C, c.G, c.twN, c.L, c.KB,
                             c.G ? (float)c.MN : 1.0f, nullptr, nullptr, c.br, c.yh);
    });
    if (rc) return rc;
    if (s0) {
        rc = state_start(ln, *st, iso, c.M, c.N, c.planes, c.qpart, c.fmap, c.prm);
        if (rc) return rc;
        rc = ln.run(ADMM_K_PREP, [&] { return launch_line_fwd(c.L, c.T, c.gl, c.flds, s, st->v0, c.spec0, c.twM, c.N); });
        if (rc) return rc;
    } else {
        hipError_t e = hipMemsetAsync(c.spec0, 0, c.planes * c.MN * 4, s);
        if (e != hipSuccess) return fail(ADMM_E_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    }
    const size_t sstride = c.planes * 2 * c.MN;   // one trajectory slot of s
    for (int it = 1; it <= maxit; ++it) {
        float2* vsave = tr.v ? tr.v + (size_t)(it - 1) * c.planes * c.N * c.L : nullptr;
        rc = ln.run(ADMM_K_COLUMN, [&] {
            return launch_column(c.N, vsave ? 7 : 6, c.gc, c.clds, s, c.spec0, c.spec1, c.C, c.G, c.twN, c.L, c.KB, 1.0f,
                                 vsave, nullptr, c.br, c.yh);
        });
        if (rc) return rc;
        if (it == maxit) break;
        Slots p = fwd_slots(it, tr.s, sstride, b0, b1);
        const int sz = it == 1 && !s0 ? 1 : 0;
        if (it == 1 && s0) p.so = s0;
        if (!iso) {
            rc = ln.run(ADMM_K_LINE, [&] {
                if (c.bt)
                    return launch_line_bt(c.L, c.Tu, c.gu, c.llds, s, c.spec1, c.spec0, p.so, p.sn, c.twM, c.N, c.prm, sz,
                                          c.nTu, c.br);
                return launch_line(c.L, c.Tu, c.gu, c.llds, s, c.spec1, c.spec0, p.so, p.sn, nullptr, c.twM, c.N, c.prm,
                                   sz, c.nTu, c.br);
            });
            if (rc) return rc;
            continue;
        }
        // isotropic: s is written in place (no halo reads of s in ISO_A); with a trajectory each
        // iteration writes its own slot and the batch norm is kept too
        rc = ln.run(ADMM_K_LINE, [&] {
            return launch_iso_a(c.L, c.T, dim3(c.N / c.T, (unsigned)c.ng), iso_a_lds(c.M, c.T), s, c.spec1, p.so, p.sn,
                                c.fmap, c.qpart, c.twM, c.N, c.gplanes, c.Gp, sz, c.ngb_k);
        });
        if (rc) return rc;
        rc = iso_norm_step(ln, c.qpart, c.fmap, c.ngb, c.MN, c.prm, tr.nrm ? tr.nrm + (size_t)(it - 1) * c.nstride : nullptr,
                           red, c.ny, c.prm_f);
        if (rc) return rc;
        rc = ln.run(ADMM_K_LINE, [&] {
            return launch_iso_b(c.L, c.T, c.gl, iso_b_lds(c.M, c.T), s, p.sn, c.fmap, nullptr, c.spec0, c.twM, c.N, c.prm,
                                c.bro);
        });
        if (rc) return rc;
    }
    return ln.run(ADMM_K_FINAL, [&] {
        return launch_line_inv(c.L, c.T, c.gl, c.flds, s, c.spec1, x_out, c.twM, c.N, c.bro, c.map_out);
    });
}

// Isotropic CU-resident solve (ADMM_PATH_RESIDENT_ISO): iteration k is one resident_iso_kernel launch (s_k, f_k ->
// s_{k+1}, q per plane; x at the last), then the 2-pass path's norm over the planes' q (iso_norm_step) -> f_{k+1}
// (and |s_{k+1}| when recording).
// Recording: s_{k+1} into trajectory slot k, read back from slot k - 1 -- the natural layout the 2-pass and
// runtime-length isotropic sweeps read.  q: planes x M x N floats (a spectrum buffer, free after PREP).
int run_resident_iso(Launcher& ln, int M, int N, size_t planes, const FwdView& v, const float* hty, float* x_out,
                     int maxit, const Traj& tr, const admm_batch_reducer* red) {
    hipStream_t s = ln.s;
    const size_t MN = (size_t)M * N, sstride = planes * 2 * MN;
    float* q = reinterpret_cast<float*>(v.spec1);
    for (int k = 0; k < maxit; ++k) {
        const float* sin = tr.s && k >= 1 ? tr.s + (size_t)(k - 1) * sstride : v.s[0];
        float* sout = tr.s ? tr.s + (size_t)k * sstride : v.s[0];
        int rc = ln.run(ADMM_K_PLANE, [&] {
            return admm::rs::launch_iso(M, N, planes, s, hty, sin, sout, v.fmap, q, x_out, v.C, v.twM, v.twN, v.prm, k, maxit);
        });
        if (rc) return rc;
        if (k + 1 == maxit) break;
        rc = iso_norm_step(ln, q, v.fmap, (int)planes, MN, v.prm, tr.nrm ? tr.nrm + (size_t)k * MN : nullptr, red);
        if (rc) return rc;
    }
    return ADMM_OK;
}

// The fused isotropic solve at 256 x 256 (plane_iso.hip), the spectrum resident in the CU: per iteration one
// plane256_iso_kernel over every plane and one iso_norm_kernel (each branch's batch norm over its own planes).
// Recording (tslot > 0): s_{k+1} into trajectory slot k, |s_{k+1}| into norm slot k (lane-native).
struct FusedIso {
    void* tabs;              // lane-native tables, per branch
    const float* prm;
    size_t planes;
    const plane::Branches* br;   // null: one solve
    float4* st;              // s state, or the trajectory slots (tslot float4 apart)
    size_t tslot;
    float2* nrm;             // |s| slots, nslot float2 apart (null: not recorded)
    size_t nslot;
    float2 *fl, *ql;         // f maps; per plane q partials (forward) / R partials (reverse)
};
// sm: a sharded batch's sum map (this shard's sums, the caller's all-reduce of the M x N map, then f)
int fused_iso_forward(Launcher& ln, const FusedIso& f, const float* y, float* x_out, bool psf, float2* hln, int maxit,
                      const admm_batch_reducer* red = nullptr, float2* sm = nullptr) {
    namespace pk = admm::plane;
    hipStream_t s = ln.s;
    for (int k = 0; k < maxit; ++k) {
        int rc = ln.run(ADMM_K_PLANE, [&] {
            return pk::launch_plane_iso(y, x_out, f.tabs, psf, hln, f.st + (k > 0 ? (size_t)(k - 1) * f.tslot : 0),
                                        f.st + (size_t)k * f.tslot, f.fl, f.ql, f.prm, k, maxit, f.planes, s, f.br);
        });
        if (rc) return rc;
        if (k + 1 == maxit) break;
        float2* nr = f.nrm ? f.nrm + (size_t)k * f.nslot : nullptr;
        if (!red) {
            rc = ln.run(ADMM_K_NORM, [&] { return pk::launch_iso_norm(f.ql, f.fl, nr, f.prm, f.planes, s, f.br); });
            if (rc) return rc;
            continue;
        }
        rc = ln.run(ADMM_K_NORM, [&] { return pk::launch_iso_norm(f.ql, f.fl, nr, f.prm, f.planes, s, nullptr, sm); });
        if (rc) return rc;
        rc = call_reducer(red, reinterpret_cast<float*>(sm), (size_t)kMultiM * kMultiN, s);
        if (rc) return rc;
        rc = ln.run(ADMM_K_NORM, [&] { return pk::launch_iso_norm(f.ql, f.fl, nr, f.prm, f.planes, s, nullptr, nullptr, sm); });
        if (rc) return rc;
    }
    return ADMM_OK;
}

// the planes of a call that one run_forward solves: all of them, or a chunk
struct PlaneRange {
    const float* y;
    float* x_out;
    size_t planes;
};
int run_forward_generic(Launcher& ln, const Call& c, const PlaneRange& r, const FwdView& v, const Traj& tr, int path,
                        const Branches& br);

// a grouped call's descriptor for the 2-pass / runtime-length kernels (C / G tables group_tab_f apart, a scalar block per
// group when it has a (lambda, rho) pair per group); a single solve: kOneSolve
Branches call_branches(const Call& c) {
    if (!c.grouped()) return kOneSolve;
    return admm::plane::grouped_branches(c.P, c.B, c.gb, c.gp, group_tab_f(c.M, c.N), c.nparam > 1 ? 4u : 0u);
}

int run_forward(Launcher& ln, const Call& c, unsigned char* ws, const Layout& lay, const Traj& tr, int fwd_path,
                bool tables, size_t p0, size_t np) {
    hipStream_t s = ln.s;
    int rc = ADMM_OK;
    const int M = c.M, N = c.N, kh = c.kh, kw = c.kw, iso = iso_batch(c.iso), maxit = c.maxit;
    const size_t MN = (size_t)M * N, planes = np ? np : c.planes();
    const float* y = c.y + p0 * MN;
    float* x_out = c.x_out + p0 * MN;
    const float* h = c.h;
    const admm::ScalarSrc& sc = c.sc;
    const admm_batch_reducer* red = c.red;
    const FwdView v = view(ws, lay, kh > 0);
    const int L = M / 2;
    const bool grp = c.grouped();
    const Branches br = call_branches(c);
    if (tables) rc = ln.run(ADMM_K_SETUP, [&] {
        const size_t lds = (size_t)(M + N) * 16 + (kh * kw <= admm::kSetupPsfLds ? (size_t)kh * kw * 4 : 0);
        const int nb = (int)(((size_t)(L + 1) * N * (kh > 0 ? admm::kSetupSplit : 1) + kThreads - 1) / kThreads);
        const int grid = nb < 1024 ? (nb < 1 ? 1 : nb) : 1024;
        if (grp) {   // every group's tables and scalars in one launch (block row = group)
            const int G = admm::plane::grouped_count(br);
            // every block computes the M + N fp64 twiddles before its bins: with many groups, fewer blocks per group
            // (down to an eighth, while 2048 blocks remain) walk more bins each -- the same arithmetic per bin
            int gx = grid;
            while (gx > 1 && gx > grid / 8 && (size_t)G * (gx / 2) >= 2048) gx /= 2;
            set_lds(admm::setup_grouped_kernel, lds);
            hipLaunchKernelGGL(admm::setup_grouped_kernel, dim3(gx, (unsigned)G), dim3(kThreads), lds, s, v.twM, v.twN,
                               v.C, v.G, h, kh, kw, M, N, sc.lam, sc.rho, br.prm_f ? G : 1, v.prm, br.tab_f, br.prm_f, tr.sig);
            return;
        }
        set_lds(admm::setup_kernel, lds);
        hipLaunchKernelGGL(admm::setup_kernel, dim3(grid), dim3(kThreads), lds, s, v.twM, v.twN, v.C, v.G, h, kh, kw, M,
                           N, sc, v.prm, tr.sig);
    });
    if (rc) return rc;
    if (maxit == 0) {
        hipError_t e = hipMemsetAsync(x_out, 0, planes * MN * 4, s);
        if (e != hipSuccess) return fail(ADMM_E_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
        return ADMM_OK;
    }

    const int path = fwd_path;
    if (generic_shape(M, N)) {   // ADMM_PATH_RESIDENT (smooth sides), _SMOOTH, _RUNTIME: the runtime-length layout
        return run_forward_generic(ln, c, PlaneRange{y, x_out, planes}, v, tr, path, br);
    }
    if (path == ADMM_PATH_FUSED) {
        // one workgroup per plane runs all K iterations (plane_kernel.hip); lane-native H^T y in
        // spec0, lane-native s in sA -- or, recording a trajectory, s_k in its own slot of tr.s
        namespace pk = admm::plane;
        if (tables) rc = ln.run(ADMM_K_SETUP, [&] {
            if (grp) return pk::launch_tables_grouped(v.C, v.G, v.F, pk::grouped_count(br), br.tab_f, s);
            return pk::launch_tables(v.C, v.G, v.F, s);
        });
        if (rc) return rc;
        if (c.st) {   // a state call: the kernel's state instance, from s_0 (v_0 first) or from the zero state
            if (c.st->in) {
                rc = state_start(ln, *c.st, false, M, N, planes, nullptr, nullptr, v.prm);
                if (rc) return rc;
            }
            return ln.run(ADMM_K_PLANE, [&] {
                return pk::launch_plane_state(y, x_out, v.F, kh > 0, v.spec0, reinterpret_cast<float4*>(v.s[0]), v.prm,
                                              maxit, planes, s, c.st->in, c.st->in ? c.st->v0 : nullptr);
            });
        }
        // a grouped solve: the same descriptor over the lane-native table blocks
        Branches bf = br;
        bf.tab_f = (unsigned)(pk::grouped_tables_bytes() / 4);
        rc = ln.run(ADMM_K_PLANE, [&] {
            if (grp && tr.s)   // a grouped recording (plane_grouped_rec.hip)
                return pk::launch_plane_grouped_rec(y, x_out, v.F, kh > 0, v.spec0, reinterpret_cast<float4*>(v.s[0]), v.prm,
                                                    maxit, planes, s, reinterpret_cast<float4*>(tr.s), bf);
            return pk::launch_plane(y, x_out, v.F, kh > 0, v.spec0, reinterpret_cast<float4*>(v.s[0]), v.prm, maxit,
                                   planes, s, tr.m ? nullptr : reinterpret_cast<float4*>(tr.s), grp ? &bf : nullptr, tr.m);
        });
        return rc;
    }
    if (path == ADMM_PATH_FUSED_ISO) {
        // isotropic at 256 x 256: the split-iteration per-plane kernels (fused_iso_forward); q partials in spec1, a
        // sharded batch's sum map in the plane-group partials' slot
        if (tables) rc = ln.run(ADMM_K_SETUP, [&] { return admm::plane::launch_tables(v.C, v.G, v.F, s); });
        if (rc) return rc;
        const size_t kE = MN / 2;   // lane-native float2 elements per plane
        const FusedIso f{v.F, v.prm, planes, nullptr, reinterpret_cast<float4*>(tr.iso_lane ? tr.s : v.s[0]),
                         tr.iso_lane ? planes * kE : 0, tr.iso_lane ? reinterpret_cast<float2*>(tr.nrm) : nullptr, kE,
                         reinterpret_cast<float2*>(v.fmap), v.spec1};
        return fused_iso_forward(ln, f, y, x_out, kh > 0, v.spec0, maxit, red, reinterpret_cast<float2*>(v.part));
    }
    TwoPass t = two_pass_single(ln, M, N, planes, line_T(M, N), v, br);
    t.bt = iso_plane(c.iso);
    if (path == ADMM_PATH_RESIDENT || path == ADMM_PATH_RESIDENT_ISO) {
        // power-of-two sides admm_resident.hip compiled: one workgroup per plane runs all K iterations (s_k into
        // the trajectory slots when recording, natural layout, as the 2-pass sweep reads them); H^T y from the
        // 2-pass kernels (line, column x conj(Sigma_c), line), the first line spectrum formed in the kernel
        float* hty = kh > 0 ? v.hty : const_cast<float*>(y);
        if (kh > 0) {
            rc = two_pass_conv(t, ADMM_K_PREP, 1, y, hty);
            if (rc) return rc;
        }
        if (path == ADMM_PATH_RESIDENT_ISO) return run_resident_iso(ln, M, N, planes, v, hty, x_out, maxit, tr, red);
        return ln.run(ADMM_K_PLANE, [&] {
            return admm::rs::launch(M, N, planes, s, hty, v.s[0], v.s[1], tr.s, planes * 2 * MN, x_out, v.C, v.twM, v.twN,
                                    v.prm, maxit);
        });
    }
    return two_pass_forward(t, y, x_out, maxit, iso != 0, tr, v.s[0], iso ? v.s[0] : v.s[1], red, c.st);
}

// ---- the runtime-length kernels (admm_generic.hip, admm_generic_bwd.hip) -----------------------------------
struct GenPass {
    int M, N, H, T, KB;
    size_t planes;
    admm::gen::FPlan pM, pN;
    dim3 gl, gc;
    size_t lfw, lup, lcol;   // LDS: line_fwd / line_inv; line_upd / iso_b and the adjoints; column
    // compile-time-plan kernels where this build has the length (admm_smooth.hip): the column pass needs
    // N, the line passes M (forward only)
    bool smc, sml;
};
GenPass gen_pass(int M, int N, size_t planes, bool smooth) {
    namespace g = admm::gen;
    GenPass p{M, N, M / 2 + 1, gen_T(M, N), gen_KB(M, N), planes, make_fplan(M), make_fplan(N)};
    p.gl = dim3(gen_nb(N, p.T), (unsigned)planes);
    p.gc = dim3((p.H + p.KB - 1) / p.KB, (unsigned)planes);
    p.lfw = gen_lds_line(M, p.T, false);
    p.lup = gen_lds_line(M, p.T, true);
    p.lcol = gen_lds_col(N, p.KB);
    set_lds(g::line_fwd_kernel, p.lfw);
    set_lds(g::line_inv_kernel, p.lfw);
    set_lds(g::column_kernel, p.lcol);
    p.smc = smooth && admm::sm::has_length(N);
    p.sml = smooth && admm::sm::has_length(M);
    return p;
}

int gen_line_fwd(Launcher& ln, const GenPass& p, const FwdView& v, int cls, const float* src, float2* dst) {
    return ln.run(cls, [&] {
        if (p.sml) return admm::sm::launch_line_fwd(p.M, p.N, p.planes, ln.s, src, dst, v.twM);
        hipLaunchKernelGGL(admm::gen::line_fwd_kernel, p.gl, dim3(256), p.lfw, ln.s, src, dst, v.twM, p.pM, p.N, p.T);
        return 0;
    });
}

int gen_line_inv(Launcher& ln, const GenPass& p, const FwdView& v, int cls, const float2* src, float* dst) {
    return ln.run(cls, [&] {
        if (p.sml) return admm::sm::launch_line_inv(p.M, p.N, p.planes, ln.s, src, dst, v.twM);
        hipLaunchKernelGGL(admm::gen::line_inv_kernel, p.gl, dim3(256), p.lfw, ln.s, src, dst, v.twM, p.pM, p.N, p.T);
        return 0;
    });
}

// dst = F^-1 [multiplier] F src with the runtime-length kernels (mode 1: conj(Sigma_c), H^T; 2: Sigma_c, H)
int gen_conv(Launcher& ln, const GenPass& p, const FwdView& v, int cls, int mode, const float* src, float* dst,
             const Branches& br = kOneSolve) {
    int rc = gen_line_fwd(ln, p, v, cls, src, v.spec0);
    if (rc) return rc;
    rc = ln.run(cls, [&] {
        if (p.smc)
            return admm::sm::launch_column(p.M, p.N, p.planes, ln.s, v.spec0, v.spec1, v.C, v.G, v.twN, 1.0f, mode,
                                           opt(ADMM_OPT_SMOOTH));
        hipLaunchKernelGGL(admm::gen::column_kernel, p.gc, dim3(256), p.lcol, ln.s, v.spec0, v.spec1, v.C, v.G, v.twN, p.pN,
                           p.H, p.KB, mode, 1.0f, (float2*)nullptr, (double*)nullptr, (float2*)nullptr, br);
        return 0;
    });
    if (rc) return rc;
    return gen_line_inv(ln, p, v, cls, v.spec1, dst);
}

int run_forward_generic(Launcher& ln, const Call& c, const PlaneRange& r, const FwdView& v, const Traj& tr, int path,
                        const Branches& br) {
    namespace g = admm::gen;
    hipStream_t s = ln.s;
    int rc = ADMM_OK;
    const int M = c.M, N = c.N, iso = iso_batch(c.iso), maxit = c.maxit;
    const bool bt = iso_plane(c.iso);
    const float* y = r.y;
    float* x_out = r.x_out;
    const size_t planes = r.planes;
    const admm_batch_reducer* red = c.red;
    const size_t MN = (size_t)M * N;
    // (a grouped solve runs the runtime-length kernels only: they take the group offsets; a state call and the
    // per-plane isotropic mode too)
    const GenPass p = gen_pass(M, N, planes, opt(ADMM_OPT_SMOOTH) != 0 && br.nbr != 0 && !c.st && !bt);
    const float* s0 = c.st ? c.st->in : nullptr;
    set_lds(g::line_upd_kernel, p.lup);
    set_lds(g::iso_b_kernel, p.lup);
    const size_t sstride = planes * 2 * MN;   // one trajectory slot of s
    // CU-resident solve (admm_resident.hip): anisotropic, no dim-2 spectra or isotropic norms recorded; it
    // forms the first line spectrum itself, so PREP only produces H^T y in space (with a PSF: F^-1 conj(Sigma_c) F y,
    // ops.jl:71-81)
    if (path == ADMM_PATH_RESIDENT || path == ADMM_PATH_RESIDENT_ISO) {   // plan_paths
        const float* hty = v.G ? v.hty : y;
        if (v.G) {
            rc = gen_conv(ln, p, v, ADMM_K_PREP, 1, y, v.hty);
            if (rc) return rc;
        }
        if (path == ADMM_PATH_RESIDENT_ISO) return run_resident_iso(ln, M, N, planes, v, hty, x_out, maxit, tr, red);
        return ln.run(ADMM_K_PLANE, [&] {
            return admm::rs::launch(M, N, planes, s, hty, v.s[0], v.s[1], tr.s, sstride, x_out, v.C, v.twM, v.twN, v.prm, maxit);
        });
    }
    // the 2-pass kernels take H^T y in the spectral domain: Y_h = conj(Sigma_c) F y (with a PSF) stored once as the
    // column pass's 2-D spectrum and added to every iteration's spectrum of rho D^T w
    float2* yh = v.yh();
    rc = gen_line_fwd(ln, p, v, ADMM_K_PREP, y, v.spec0);
    if (rc) return rc;
    rc = ln.run(ADMM_K_PREP, [&] {
        hipLaunchKernelGGL(g::column_kernel, p.gc, dim3(256), p.lcol, s, v.spec0, v.spec1, v.C, v.G, v.twN, p.pN, p.H, p.KB,
                           32 | 1, v.G ? (float)MN : 1.0f, (float2*)nullptr, (double*)nullptr, yh, br);
        return 0;
    });
    if (rc) return rc;
    if (s0) {   // a warm state call: the line spectrum of v_0 = rho D^T (z_0 - u_0)
        rc = state_start(ln, *c.st, iso != 0, M, N, planes, v.part, v.fmap, v.prm);
        if (rc) return rc;
        rc = gen_line_fwd(ln, p, v, ADMM_K_PREP, c.st->v0, v.spec0);
        if (rc) return rc;
    } else {
        hipError_t e = hipMemsetAsync(v.spec0, 0, planes * (size_t)p.H * N * 8, s);   // iteration 1: w = 0
        if (e != hipSuccess) return fail(ADMM_E_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    }
    const int ng = iso_ngroups(planes);
    for (int it = 1; it <= maxit; ++it) {
        // trajectory for h_bar: the dim-2 spectrum of iteration it before the multiply
        float2* vsave = tr.v ? tr.v + (size_t)(it - 1) * planes * N * p.H : nullptr;
        rc = ln.run(ADMM_K_COLUMN, [&] {
            if (p.smc && !vsave)
                return admm::sm::launch_column(M, N, planes, s, v.spec0, v.spec1, v.C, v.G, v.twN, 1.0f, 0,
                                               opt(ADMM_OPT_SMOOTH), yh);
            hipLaunchKernelGGL(g::column_kernel, p.gc, dim3(256), p.lcol, s, v.spec0, v.spec1, v.C, v.G, v.twN, p.pN, p.H,
                               p.KB, (vsave ? 4 : 0) | 16, 1.0f, vsave, (double*)nullptr, yh, br);
            return 0;
        });
        if (rc) return rc;
        const bool last = it == maxit;
        rc = gen_line_inv(ln, p, v, last ? ADMM_K_FINAL : ADMM_K_LINE, v.spec1, last ? x_out : v.xg);
        if (rc) return rc;
        if (last) break;
        Slots sl = fwd_slots(it, tr.s, sstride, v.s[0], iso ? v.s[0] : v.s[1]);
        const int first = it == 1 && !s0 ? 1 : 0;
        if (it == 1 && s0) sl.so = s0;
        if (!iso) {
            rc = ln.run(ADMM_K_LINE, [&] {
                if (bt)
                    return launch_gen_line_upd_bt(p.gl, p.lup, s, v.xg, sl.so, sl.sn, v.spec0, v.twM, p.pM, N, p.T, v.prm,
                                                  first, br);
                if (p.sml)
                    return admm::sm::launch_line_upd(M, N, planes, s, v.xg, sl.so, sl.sn, nullptr, v.spec0, v.twM, v.prm,
                                                     first);
                hipLaunchKernelGGL(g::line_upd_kernel, p.gl, dim3(256), p.lup, s, v.xg, sl.so, sl.sn, (const float*)nullptr,
                                   v.spec0, v.twM, p.pM, N, p.T, v.prm, first, br);
                return 0;
            });
            if (rc) return rc;
            continue;
        }
        rc = ln.run(ADMM_K_LINE, [&] {
            hipLaunchKernelGGL(g::iso_a_kernel, dim3(gen_nb(N, p.T), ng), dim3(256), (size_t)p.T * M * 4, s, v.xg, sl.so,
                               sl.sn, v.fmap, v.part, M, N, (int)planes, iso_group(planes), p.T, first);
        });
        if (rc) return rc;
        rc = iso_norm_step(ln, v.part, v.fmap, ng, MN, v.prm, tr.nrm ? tr.nrm + (size_t)(it - 1) * MN : nullptr, red);
        if (rc) return rc;
        rc = ln.run(ADMM_K_LINE, [&] {
            hipLaunchKernelGGL(g::iso_b_kernel, p.gl, dim3(256), p.lup, s, sl.sn, v.fmap, (const float*)nullptr, v.spec0,
                               v.twM, p.pM, N, p.T, v.prm);
        });
        if (rc) return rc;
    }
    return ADMM_OK;
}

// out[c] = sum over the n rows of column c of part (n x w row-major), in a fixed order
void launch_reduce_cols(hipStream_t s, const double* part, double* out, int n, int w, double* tmp) {
    const int chunk = 2048;
    const int parts = (n + chunk - 1) / chunk;
    if (parts <= 1) {
        hipLaunchKernelGGL(admm::reduce_cols_kernel, dim3(w), dim3(kThreads), 0, s, part, out, n, w);
        return;
    }
    const int ch = (n + (parts < kRedParts ? parts : kRedParts) - 1) / (parts < kRedParts ? parts : kRedParts);
    const int g = (n + ch - 1) / ch;
    hipLaunchKernelGGL(admm::reduce_cols_part_kernel, dim3(w, g), dim3(kThreads), 0, s, part, tmp, n, w, ch);
    hipLaunchKernelGGL(admm::reduce_cols_kernel, dim3(w), dim3(kThreads), 0, s, tmp, out, g, w);
}

int launch_line_adj(int L, int T, dim3 g, size_t lds, hipStream_t s, const float2* spec1, const float* sk1,
                    const float* sk, const float* xK, const float* sb_in, float* sb_out, float* vsum, float2* spec0,
                    double* part, const float2* twM, int N, const float* prm, int first_k, int last_k, bool ln,
                    const Branches& br = kOneSolve, size_t pbs = 0) {
    if (br.nbr == 0)   // a grouped solve: the plane's group scalars, rows by plane
        return launch_line_adj_grouped(L, T, g, lds, s, spec1, sk1, sk, xK, sb_in, sb_out, vsum, spec0, part, twM, N, prm,
                                       first_k, last_k, ln, br);
    if (ln) {   // trajectory in the fused kernel's lane-native layout (M = 256)
#define X(l, t)                                                                                                \
        if (L == l && T == t) {                                                                                \
            set_lds(line_adj_kernel<l, t, true>, lds);                                                         \
            line_adj_kernel<l, t, true><<<g, kThreads, lds, s>>>(spec1, sk1, sk, xK, sb_in, sb_out, vsum, spec0, \
                                                                  part, twM, N, prm, first_k, last_k);    \
            return 0;                                                                                          \
        }
        X(128, 2) X(128, 4) X(128, 8) X(128, 16)
#undef X
        return -1;
    }
#define X(l, t)                                                                                                \
    if (L == l && T == t) {                                                                                    \
        set_lds(line_adj_kernel<l, t>, lds);                                                                   \
        line_adj_kernel<l, t><<<g, kThreads, lds, s>>>(spec1, sk1, sk, xK, sb_in, sb_out, vsum, spec0, part, twM, \
                                                        N, prm, first_k, last_k, br, pbs);               \
        return 0;                                                                                              \
    }
    ADMM_LT_CASES(X)
#undef X
    return -1;
}

// br / ngb / pbs: several branches (planes per branch, plane groups per branch, doubles between the branches'
// partial-row blocks)
int launch_iso_adj_a(int L, int T, dim3 g, size_t lds, hipStream_t s, const float2* spec1, const float* sk1,
                     const float* sk, const float* xK, const float* nrm1, const float* sb_in, float* wbar, float* vsum,
                     float* rpartial, double* part, const float2* twM, int N, int planes, int G, const float* prm,
                     int first_k, int last_k, const Branches& br = kOneSolve, int ngb = 0, size_t pbs = 0) {
#define X(l, t)                                                                                                 \
    if (L == l && T == t) {                                                                                     \
        set_lds(iso_adj_a_kernel<l, t>, lds);                                                                   \
        iso_adj_a_kernel<l, t><<<g, kThreads, lds, s>>>(spec1, sk1, sk, xK, nrm1, nullptr, sb_in, wbar, vsum,  \
                                                         rpartial, part, twM, N, planes, G, prm, first_k,  \
                                                         last_k, br, ngb, pbs);                                 \
        return 0;                                                                                               \
    }
    ADMM_LT_CASES(X)
#undef X
    return -1;
}

int launch_iso_adj_b(int L, int T, dim3 g, size_t lds, hipStream_t s, const float* wbar, const float* sb_in,
                     const float* sk1, const float* nrm1, const float* Rmap, float* sb_out, float2* spec0,
                     const float2* twM, int N, const float* prm, const Branches& br = kOneSolve) {
#define X(l, t)                                                                                                 \
    if (L == l && T == t) {                                                                                     \
        set_lds(iso_adj_b_kernel<l, t>, lds);                                                                   \
        iso_adj_b_kernel<l, t><<<g, kThreads, lds, s>>>(wbar, sb_in, sk1, nrm1, Rmap, sb_out, spec0, twM, N,    \
                                                         prm, br);                                              \
        return 0;                                                                                               \
    }
    ADMM_LT_CASES(X)
#undef X
    return -1;
}

// ---- reverse sweeps -------------------------------------------------------------------------------------------
// Step k = K .. 1 reads s_{k-1} (sk1) and, for rho_bar, s_k (skk) from the trajectory, |s_{k-1}| (isotropic),
// sbar_{k+1} from one sbar buffer (none at k = K) and writes sbar_k to the other; its (rho_bar, tau_bar) partial
// rows start at row (K - k) x rows.
struct RevStep {
    const float *sk1, *skk, *nrm1, *sbi;
    float* sbo;
    double* rp;
};
RevStep rev_step(int k, int K, const SweepBufs& b, size_t sstride, size_t nstride, int rows) {
    return RevStep{k >= 2 ? b.traj + (size_t)(k - 2) * sstride : nullptr,
                   k < K ? b.traj + (size_t)(k - 1) * sstride : nullptr,
                   b.nrm && k >= 2 ? b.nrm + (size_t)(k - 2) * nstride : nullptr,
                   k < K ? b.sb[k & 1] : nullptr,
                   b.sb[(k & 1) ^ 1],
                   b.part + (size_t)(K - k) * rows * 2};
}

// The 2-pass reverse sweep: the line transform of x_bar, then per step the column pass (with h_bar: the recorded
// spectrum of the step and the Q accumulators) and the line adjoint -- or, isotropic, ISO_ADJ_A (plane groups) ->
// ISO_ADJ_R (batch R map, tau_bar) -> ISO_ADJ_B (per plane); k = 1 launches no ISO_ADJ_R or _B.
// ln_traj: the trajectory is in the fused kernel's lane-native layout (M = 256, anisotropic)
// A grouped solve (c.br.nbr = 0): the column pass takes the plane's group C table and the line adjoint its group
// scalars; the isotropic adjoint kernels keep c.bro -- an isotropic grouped solve has one (lambda, rho) pair, in block 0.
int two_pass_reverse(const TwoPass& c, const SweepBufs& b, const float* x_bar, int K, bool iso, bool ln_traj,
                     const admm_batch_reducer* red = nullptr) {
    Launcher& ln = c.ln;
    hipStream_t s = ln.s;
    const size_t sstride = c.planes * 2 * c.MN;
    const size_t alds = line_lds(c.M, c.T) + 8 * 16;
    int rc = ln.run(ADMM_K_PREP, [&] {
        return launch_line_fwd(c.L, c.T, c.gl, c.flds, s, x_bar, c.spec0, c.twM, c.N, c.bro, c.map_out);
    });
    if (rc) return rc;
    for (int k = K; k >= 1; --k) {
        float2* vs = b.v ? b.v + (size_t)(k - 1) * c.planes * c.N * c.L : nullptr;
        rc = ln.run(ADMM_K_COLUMN, [&] {
            return launch_column(c.N, b.v ? 4 : 0, c.gc, c.clds, s, c.spec0, c.spec1, c.C, c.G, c.twN, c.L, c.KB, 1.0f, vs,
                                 b.Qp, c.br);
        });
        if (rc) return rc;
        const RevStep r = rev_step(k, K, b, sstride, c.nstride, c.rows);
        const float* skk = b.xK ? r.skk : nullptr;   // s_k and D x_K enter rho_bar's <D vbar, D x_k> only
        if (!iso) {
            rc = ln.run(ADMM_K_ADJ, [&] {
                if (c.bt)
                    return launch_line_adj_bt(c.L, c.T, c.gl, alds, s, c.spec1, r.sk1, skk, b.xK, r.sbi, r.sbo, b.vsum,
                                              c.spec0, r.rp, c.twM, c.N, c.prm, k == 1 ? 1 : 0, k == K ? 1 : 0, c.br);
                return launch_line_adj(c.L, c.T, c.gl, alds, s, c.spec1, r.sk1, skk, b.xK, r.sbi, r.sbo, b.vsum, c.spec0,
                                       r.rp, c.twM, c.N, c.prm, k == 1 ? 1 : 0, k == K ? 1 : 0, ln_traj, c.br, c.pbs);
            });
            if (rc) return rc;
            continue;
        }
        rc = ln.run(ADMM_K_ADJ, [&] {
            return launch_iso_adj_a(c.L, c.T, dim3(c.N / c.T, (unsigned)c.ng), iso_a_lds(c.M, c.T) + 8 * 16, s, c.spec1,
                                    r.sk1, skk, b.xK, r.nrm1, r.sbi, b.wbar, b.vsum, b.Rpart, r.rp, c.twM, c.N, c.gplanes,
                                    c.Gp, c.prm, k == 1 ? 1 : 0, k == K ? 1 : 0, c.bro, c.ngb_k, c.pbs);
        });
        if (rc) return rc;
        if (k == 1) break;
        rc = ln.run(ADMM_K_NORM, [&] {
            hipLaunchKernelGGL(admm::iso_adj_r_kernel, dim3(kIsoAdjRBlocks, c.ny), dim3(kThreads), 0, s, b.Rpart, b.Rmap,
                               r.nrm1, c.ngb, c.MN, c.prm, r.rp + (size_t)c.r_off * 2, c.prm_f, c.pbs);
        });
        if (rc) return rc;
        // sharded batch: tau_bar above used this shard's R (shard contributions add up, like every other
        // parameter gradient); sbar needs the whole batch's R
        if (red) {
            rc = call_reducer(red, b.Rmap, c.MN, s);
            if (rc) return rc;
        }
        rc = ln.run(ADMM_K_ADJ, [&] {
            return launch_iso_adj_b(c.L, c.T, c.gl, iso_b_lds(c.M, c.T), s, b.wbar, r.sbi, r.sk1, r.nrm1, b.Rmap, r.sbo,
                                    c.spec0, c.twM, c.N, c.prm, c.bro);
        });
        if (rc) return rc;
    }
    return ADMM_OK;
}

// The runtime-length reverse sweep (admm_generic_bwd.hip): per step column, line inverse -> vbar_k in HBM (the
// forward's x slot), then the line adjoint (aniso) or ISO_ADJ_A -> ISO_ADJ_R -> ISO_ADJ_B.  These kernels take s_k and
// x_K (rho_bar's terms) whether or not rho_bar is wanted.  br: a grouped solve's descriptor (the column pass and the
// line adjoint look the plane's group up; the isotropic kernels read the one scalar block).
int runtime_reverse(Launcher& ln, const GenPass& p, const FwdView& v, const SweepBufs& b, const float* x_bar,
                    const float* xK, int K, bool iso, int rows, int r_off, const admm_batch_reducer* red,
                    const Branches& br = kOneSolve, bool bt = false) {
    namespace g = admm::gen;
    hipStream_t s = ln.s;
    const int M = p.M, N = p.N;
    const size_t MN = (size_t)M * N, sstride = p.planes * 2 * MN;
    const int ngi = iso_ngroups(p.planes);
    set_lds(g::line_adj_kernel, p.lup);
    set_lds(g::iso_adj_b_kernel, p.lup);
    float* vb = v.xg;
    int rc = gen_line_fwd(ln, p, v, ADMM_K_PREP, x_bar, v.spec0);
    if (rc) return rc;
    for (int k = K; k >= 1; --k) {
        float2* vs = b.v ? b.v + (size_t)(k - 1) * p.planes * N * p.H : nullptr;
        rc = ln.run(ADMM_K_COLUMN, [&] {
            hipLaunchKernelGGL(g::column_kernel, p.gc, dim3(256), p.lcol, s, v.spec0, v.spec1, v.C, v.G, v.twN, p.pN, p.H,
                               p.KB, b.v ? 8 : 0, 1.0f, vs, b.Qp, (float2*)nullptr, br);
        });
        if (rc) return rc;
        rc = gen_line_inv(ln, p, v, ADMM_K_LINE, v.spec1, vb);
        if (rc) return rc;
        const RevStep r = rev_step(k, K, b, sstride, MN, rows);
        if (!iso) {
            rc = ln.run(ADMM_K_ADJ, [&] {
                if (bt)   // ADMM_ISO_PLANE
                    return launch_gen_line_adj_bt(p.gl, p.lup, s, vb, r.sk1, r.skk, xK, r.sbi, r.sbo, b.vsum, v.spec0, r.rp,
                                                  v.twM, p.pM, N, p.T, v.prm, br);
                hipLaunchKernelGGL(g::line_adj_kernel, p.gl, dim3(256), p.lup, s, vb, r.sk1, r.skk, xK, r.sbi, r.sbo,
                                   b.vsum, v.spec0, r.rp, v.twM, p.pM, N, p.T, v.prm, br);
                return 0;
            });
            if (rc) return rc;
            continue;
        }
        rc = ln.run(ADMM_K_ADJ, [&] {
            hipLaunchKernelGGL(g::iso_adj_a_kernel, dim3(gen_nb(N, p.T), (unsigned)ngi), dim3(256), (size_t)p.T * M * 4, s,
                               vb, r.sk1, r.skk, xK, r.nrm1, r.sbi, b.wbar, b.vsum, b.Rpart, r.rp, M, N, (int)p.planes,
                               iso_group(p.planes), p.T, v.prm);
        });
        if (rc) return rc;
        if (k == 1) break;
        rc = ln.run(ADMM_K_NORM, [&] {
            hipLaunchKernelGGL(admm::iso_adj_r_kernel, dim3(kIsoAdjRBlocks), dim3(kThreads), 0, s, b.Rpart, b.Rmap, r.nrm1,
                               ngi, MN, v.prm, r.rp + (size_t)r_off * 2);
        });
        if (rc) return rc;
        if (red) {
            rc = call_reducer(red, b.Rmap, MN, s);
            if (rc) return rc;
        }
        rc = ln.run(ADMM_K_ADJ, [&] {
            hipLaunchKernelGGL(g::iso_adj_b_kernel, p.gl, dim3(256), p.lup, s, b.wbar, r.sbi, r.sk1, r.nrm1, b.Rmap, r.sbo,
                               v.spec0, v.twM, p.pM, N, p.T, v.prm);
        });
        if (rc) return rc;
    }
    return ADMM_OK;
}

// The fused reverse sweep: one workgroup per plane runs all K steps (plane256_adj_kernel).  traj: the forward's s_k, or
// (masks) their ST mask bits; with rho_bar (xK given) D x_K goes to dxK first, lane-native: it and s_k enter rho_bar's
// <D vbar, D x_k> only.  part: 2 doubles per plane.
int fused_reverse(Launcher& ln, const float* x_bar, const void* tabs, const void* traj, bool masks, const float* xK,
                  float4* dxK, float4* sbar, float2* vsl, float* vout, double* part, const float* prm, int K, size_t planes,
                  const plane::Branches* br = nullptr) {
    namespace pk = admm::plane;
    hipStream_t s = ln.s;
    if (!xK) dxK = nullptr;
    if (dxK) {
        int rc = ln.run(ADMM_K_PREP, [&] { return pk::launch_dx_lane(xK, dxK, planes, s, br); });
        if (rc) return rc;
    }
    return ln.run(ADMM_K_ADJ, [&] {
        return pk::launch_plane_adj(x_bar, tabs, traj, dxK, sbar, vsl, vout, part, prm, K, planes, s, br, masks);
    });
}

// The fused isotropic sweep (plane_iso.hip) over f's planes: per step one plane256_isoadj_kernel (B phase of step
// k + 1, column phase, A phase of step k) and, for k >= 2, one iso_radj_kernel (R_k per branch, tau_bar rows: step k's
// at (K - k) x 512 of each branch's block, part_branch doubles apart).  f.ql: the per plane R partials.
int fused_iso_reverse(Launcher& ln, const FusedIso& f, const float* x_bar, float2* vbuf, float4* sbar, float2* rmap,
                      float2* vsl, float* vout, double* part, size_t part_branch, int K,
                      const admm_batch_reducer* red = nullptr) {
    namespace pk = admm::plane;
    hipStream_t s = ln.s;
    for (int k = K; k >= 1; --k) {
        int rc = ln.run(ADMM_K_ADJ, [&] {
            return pk::launch_plane_isoadj(x_bar, f.tabs, f.st, f.tslot, f.nrm, f.nslot, vbuf, sbar, rmap, f.ql, vsl, vout,
                                           f.prm, k, K, f.planes, s, f.br);
        });
        if (rc) return rc;
        if (k == 1) break;
        rc = ln.run(ADMM_K_NORM, [&] {
            return pk::launch_iso_radj(f.ql, rmap, f.nrm + (size_t)(k - 2) * f.nslot, part + (size_t)(K - k) * 512 * 2,
                                       part_branch, f.prm, f.planes, s, f.br);
        });
        if (rc) return rc;
        // sharded batch: tau_bar above used this shard's R (shard contributions add up); sbar needs the whole
        // batch's R
        if (red) {
            rc = call_reducer(red, reinterpret_cast<float*>(rmap), (size_t)kMultiM * kMultiN, s);
            if (rc) return rc;
        }
    }
    return ADMM_OK;
}

// One-grid call: each branch's partial rows (bstride doubles apart) -> its (rho_bar, tau_bar) sums -> lambda_bar[i],
// rho_bar[i]; then y_bar = the sum of the branches' Vsum (n floats each)
int branch_grads(Launcher& ln, const MultiView& v, size_t bstride, int rows, float* lambda_bar, float* rho_bar,
                 const float* vsum, float* y_bar, size_t n, int nbr) {
    hipStream_t s = ln.s;
    for (int i = 0; i < nbr; ++i) {
        int rc = ln.run(ADMM_K_FINAL, [&] { launch_reduce_cols(s, v.part + (size_t)i * bstride, v.rt + 2 * i, rows, 2, v.rtmp); });
        if (rc) return rc;
        rc = ln.run(ADMM_K_FINAL, [&] {
            hipLaunchKernelGGL(admm::grads_final_kernel, dim3(1), dim3(64), 0, s, v.rt + 2 * i, (const double*)nullptr,
                               (const double*)nullptr, 0, v.prm + 4 * i, lambda_bar ? lambda_bar + i : nullptr,
                               rho_bar ? rho_bar + i : nullptr, (float*)nullptr);
        });
        if (rc) return rc;
    }
    if (!y_bar) return ADMM_OK;
    return ln.run(ADMM_K_FINAL, [&] {
        hipLaunchKernelGGL(admm::branch_sum_kernel, dim3(1024), dim3(kThreads), 0, s, vsum, y_bar, n, nbr);
    });
}

#define HIPCHK(call)                                                                                   \
    do {                                                                                               \
        const hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) return fail(ADMM_E_HIP, "%s: %s", #call, hipGetErrorString(e_));         \
    } while (0)

// group-segmented column sums of partial rows [step][plane][blk] x w -> out[group][w] (reduce_groups_kernel)
void launch_reduce_groups(hipStream_t s, const double* part, double* out, int nsteps, size_t step_rows, int nblk, int w,
                          const Branches& br, int groups, int split, double* tmp) {
    const long long n = ((long long)nsteps * admm::group_planes(br) * nblk + split - 1) / split;
    const int nt = n <= 64 ? 64 : kThreads;
    hipLaunchKernelGGL(admm::reduce_groups_kernel, dim3(w, groups, split), dim3(nt), 0, s, part, split > 1 ? tmp : out,
                       nsteps, step_rows, nblk, w, br);
    if (split > 1)
        hipLaunchKernelGGL(admm::reduce_groups_fin_kernel, dim3((groups * w + 255) / 256), dim3(256), 0, s, tmp, out, split,
                           w, groups * w);
}

// How grouping enters the adjoint driver, consulted where a grouped call differs from a single solve: the kernels'
// descriptor, G PSF groups, nparam (lambda, rho) pairs and the parts the group-segmented sums are split in.  A single
// solve is kOneSolve with one group; a grouped call with one group still runs the grouped kernels.  The workspace of
// a grouped call is a BwdLayout whose table, scalar, sig, Q, hcorr, hA and rt slots are the per-group blocks
// (make_grouped_bwd_layout).
struct Grouping {
    Branches br;
    int G, nparam;
    unsigned tab_f;
    int split_rt, split_h;
    double* gtmp;
    bool on() const { return br.nbr == 0; }
};
Grouping grouping_of(const Call& c, const BwdLayout& bl, unsigned char* ws) {
    if (!c.grouped()) return Grouping{kOneSolve, 1, 1, 0u, 1, 1, nullptr};
    return Grouping{call_branches(c), c.groups(), c.nparam, group_tab_f(c.M, c.N), bl.split_rt, bl.split_h,
                    at<double>(ws, bl.gtmp)};
}

// Assembly of the gradients: the (rho_bar, tau_bar) rows, y_bar = H Vsum (or Vsum), h_bar = the correlation of Vsum
// with y and the spectral term from Q, then lambda_bar / rho_bar / h_bar -- per group for a grouped call (every plane
// with its group's tables; admm_backward.hip, last section).
// conv: the path's spectral convolution (two_pass_conv or gen_conv) of Vsum into y_bar; copy: y_bar is not already
// Vsum (the fused sweeps write it there)
template <typename Conv>
int assemble_grads(Launcher& ln, const BwdView& v, const BwdLayout& bl, const Call& c, const Grads& g, const Grouping& gr,
                   int red_rows, bool copy, Conv&& conv) {
    hipStream_t s = ln.s;
    const SweepBufs& b = v.b;
    const int M = c.M, N = c.N, kh = c.kh, kw = c.kw, ntaps = kh * kw;
    const size_t planes = c.planes();
    // (rho_bar, tau_bar): every row into one pair -- or, anisotropic grouped, per (lambda, rho) pair its planes' rows
    const Branches all{c.P * c.B, 0, c.P, 0u, 0u, 0, 0};   // one pair for every group: one segment of all planes
    int rc = ln.run(ADMM_K_FINAL, [&] {
        if (!gr.on() || iso_batch(c.iso)) launch_reduce_cols(s, b.part, v.rt, red_rows, 2, v.rtmp);
        else launch_reduce_groups(s, b.part, v.rt, c.maxit, (size_t)bl.nblk_line, bl.nblk_line / (int)planes, 2,
                                  gr.nparam > 1 ? gr.br : all, gr.nparam, gr.split_rt, gr.gtmp);
    });
    if (rc) return rc;
    if (kh > 0 && b.vsum) {
        if (g.y_bar) {   // y_bar = H vsum  (centred circular convolution, spectrally; a plane's own group's H)
            rc = conv(b.vsum, g.y_bar);
            if (rc) return rc;
        }
        if (g.h_bar) {
            rc = ln.run(ADMM_K_FINAL, [&] {
                const size_t lds = (size_t)(2 * bl.TY + kw - 1) * M * 4;
                set_lds(admm::hbar_corr_kernel, lds);
                hipLaunchKernelGGL(admm::hbar_corr_kernel, dim3(N / bl.TY, (unsigned)planes), dim3(kThreads), lds, s,
                                   b.vsum, c.y, v.hpart, M, N, kh, kw, bl.TY);
            });
            if (rc) return rc;
            rc = ln.run(ADMM_K_FINAL, [&] {
                if (!gr.on()) launch_reduce_cols(s, v.hpart, v.hcorr, bl.nblk_corr, ntaps, v.rtmp);
                else launch_reduce_groups(s, v.hpart, v.hcorr, 1, 0, N / bl.TY, ntaps, gr.br, gr.G, gr.split_h, gr.gtmp);
            });
            if (rc) return rc;
            const int nq = (M / 2 + 1) * N;
            rc = ln.run(ADMM_K_FINAL, [&] {
                if (!gr.on())
                    hipLaunchKernelGGL(admm::reduce_planes_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, b.Qp, v.Q,
                                       (int)planes, nq);
                else
                    hipLaunchKernelGGL(admm::reduce_planes_grouped_kernel, dim3((nq + 255) / 256, (unsigned)gr.G), dim3(256),
                                       0, s, b.Qp, v.Q, nq, gr.br);
            });
            if (rc) return rc;
            rc = ln.run(ADMM_K_FINAL, [&] {
                if (!gr.on())
                    hipLaunchKernelGGL(admm::hbarA_kernel, dim3(ntaps), dim3(kThreads), 0, s, v.Q, v.f.C, v.sig, kh, M, N, v.hA);
                else
                    hipLaunchKernelGGL(admm::hbarA_grouped_kernel, dim3(ntaps, (unsigned)gr.G), dim3(kThreads), 0, s, v.Q,
                                       v.f.C, v.sig, kh, ntaps, M, N, v.hA, gr.tab_f);
            });
            if (rc) return rc;
        }
    } else if (copy && g.y_bar) {
        HIPCHK(hipMemcpyAsync(g.y_bar, b.vsum, planes * (size_t)M * N * 4, hipMemcpyDeviceToDevice, s));
    }
    return ln.run(ADMM_K_FINAL, [&] {
        const int nt = ntaps > 1 ? ntaps : 1;
        const bool hb = g.h_bar && kh > 0;
        if (!gr.on())
            hipLaunchKernelGGL(admm::grads_final_kernel, dim3((nt + 255) / 256), dim3(256), 0, s, v.rt, v.hcorr, v.hA, ntaps,
                               v.f.prm, g.lambda_bar, g.rho_bar, hb ? g.h_bar : nullptr);
        else
            hipLaunchKernelGGL(admm::grads_final_grouped_kernel, dim3((nt + 255) / 256, (unsigned)gr.G), dim3(256), 0, s,
                               v.rt, hb ? v.hcorr : nullptr, hb ? v.hA : nullptr, ntaps, v.f.prm, gr.br.prm_f, gr.nparam,
                               g.lambda_bar, g.rho_bar, hb ? g.h_bar : nullptr);
    });
}

// The adjoint of a single or a grouped call: one recording forward, one reverse sweep over every plane (a grouped
// call's with its group's tables and scalars; plan: plan_paths'), then the assembly.
int launch_backward(int phases, const Call& c, const Grads& g, const PathPlan& plan, const BwdLayout& bl) {
    int rc = ADMM_OK;
    unsigned char* ws = static_cast<unsigned char*>(c.workspace);
    hipStream_t s = reinterpret_cast<hipStream_t>(c.stream);
    Launcher ln{s, g_prof.on, {}};
    const int M = c.M, N = c.N, kh = c.kh, K = c.maxit;
    const bool iso = iso_batch(c.iso), bt = iso_plane(c.iso);
    const size_t planes = c.planes(), MN = (size_t)M * N;
    const Grouping gr = grouping_of(c, bl, ws);
    if (K == 0) {
        if (phases & 2) {
            if (g.y_bar) HIPCHK(hipMemsetAsync(g.y_bar, 0, planes * MN * 4, s));
            if (g.h_bar && kh > 0) HIPCHK(hipMemsetAsync(g.h_bar, 0, (size_t)gr.G * kh * c.kw * 4, s));
            if (g.lambda_bar) HIPCHK(hipMemsetAsync(g.lambda_bar, 0, (size_t)gr.nparam * 4, s));
            if (g.rho_bar) HIPCHK(hipMemsetAsync(g.rho_bar, 0, (size_t)gr.nparam * 4, s));
        }
        if (phases & 1) HIPCHK(hipMemsetAsync(c.x_out, 0, planes * MN * 4, s));
        return ln.finish();
    }
    // Vsum = sum_k vbar_k feeds y_bar and the h_bar correlation only: without either the sweeps skip it
    const bool want_v = g.y_bar != nullptr || (g.h_bar != nullptr && kh > 0);
    const BwdView v = view(ws, bl, kh > 0, iso, plan.want_h, want_v, g.rho_bar ? c.x_out : nullptr);
    const SweepBufs& b = v.b;
    // ---- forward with trajectory (s_k natural or, from the fused kernel, lane-native; with h_bar the dim-2 spectra
    // and the PSF spectrum, a grouped call's of every group) ----
    Traj tr;
    tr.s = const_cast<float*>(b.traj);
    tr.m = plan.masks && !iso ? at<unsigned>(ws, bl.traj_s) : nullptr;
    tr.iso_lane = plan.iso_lane;   // the fused isotropic sweep (no mask bits: s itself is needed)
    tr.v = b.v;
    tr.sig = v.sig;
    tr.nrm = const_cast<float*>(b.nrm);
    if (phases & 1) {
        rc = run_forward(ln, c, ws, bl.f, tr, plan.fwd);
        if (rc) return rc;
    }
    if (!(phases & 2)) return ln.finish();
    // replay (phase 2 alone): the recording's tables and {tau, rho, lambda} blocks are still in the workspace and are
    // used as they are -- the reverse sweep must differentiate the trajectory that was recorded, even if a
    // device-resident lambda / rho has changed since (host values were checked against the tag)
    // ---- reverse sweep ----
    // the fused sweeps (single solves only) write Vsum straight into y_bar without a PSF
    float* vout = !want_v ? nullptr : kh > 0 ? b.vsum : g.y_bar;
    const bool fused = plan.bwd == ADMM_PATH_SWEEP_FUSED || plan.bwd == ADMM_PATH_SWEEP_FUSED_ISO;
    int red_rows = K * bl.nblk_line;   // rows of (rho_bar, tau_bar) partials
    if (!fused) {
        if (b.vsum) HIPCHK(hipMemsetAsync(b.vsum, 0, planes * MN * 4, s));
        // k = 1 launches no ISO_ADJ_R: its partial rows must read as zero
        if (iso) HIPCHK(hipMemsetAsync(b.part, 0, (size_t)K * bl.nblk_line * 2 * 8, s));
        if (b.Qp) HIPCHK(hipMemsetAsync(b.Qp, 0, planes * (size_t)(M / 2 + 1) * N * 8, s));
    }
    const bool gen = generic_shape(M, N);   // runtime-length path (admm_generic.hip, admm_generic_bwd.hip)
    const GenPass gpass = gen ? gen_pass(M, N, planes, false) : GenPass{};
    auto grid = [&] {   // the 2-pass grid of the sweep and of y_bar = H Vsum (power-of-two shapes)
        TwoPass t = two_pass_single(ln, M, N, planes, bwd_line_T(M, N, iso), v.f, gr.br);
        t.rows = bl.nblk_line, t.r_off = bl.nblk_isoA;
        t.bt = bt;
        return t;
    };
    switch (plan.bwd) {
        case ADMM_PATH_SWEEP_FUSED:   // D x_K in the second sbar buffer, lane-native Vsum in spec0
            rc = fused_reverse(ln, g.x_bar, v.f.F, b.traj, tr.m != nullptr, b.xK, reinterpret_cast<float4*>(b.sb[1]),
                               reinterpret_cast<float4*>(b.sb[0]), v.f.spec0, vout, b.part, v.f.prm, K, planes);
            red_rows = (int)planes;
            break;
        case ADMM_PATH_SWEEP_FUSED_ISO: {
            // vbar in the wbar slot, per plane R partials in spec1 (the forward's q partials, free now), lane-native
            // Vsum in spec0 (the forward's H^T y, free now); rows of step k at (K - k) x 512
            const size_t kE = MN / 2;   // lane-native float2 elements per plane
            red_rows = (K > 1 ? K - 1 : 1) * 512;
            HIPCHK(hipMemsetAsync(b.part, 0, (size_t)red_rows * 2 * 8, s));
            const FusedIso f{v.f.F, v.f.prm, planes, nullptr, reinterpret_cast<float4*>(tr.s), planes * kE,
                             reinterpret_cast<float2*>(tr.nrm), kE, nullptr, v.f.spec1};
            rc = fused_iso_reverse(ln, f, g.x_bar, at<float2>(ws, bl.wbar), reinterpret_cast<float4*>(b.sb[0]),
                                   at<float2>(ws, bl.Rmap), v.f.spec0, vout, b.part, 0, K, c.red);
            break;
        }
        case ADMM_PATH_SWEEP_RUNTIME:
        case ADMM_PATH_SWEEP_RUNTIME_ISO:
            rc = runtime_reverse(ln, gpass, v.f, b, g.x_bar, c.x_out, K, iso, bl.nblk_line, bl.nblk_isoA, c.red, gr.br, bt);
            break;
        default:
            rc = two_pass_reverse(grid(), b, g.x_bar, K, iso, plan.ln_traj, c.red);
    }
    if (rc) return rc;
    // ---- assembly ----
    rc = assemble_grads(ln, v, bl, c, g, gr, red_rows, !fused, [&](const float* src, float* dst) {
        return gen ? gen_conv(ln, gpass, v.f, ADMM_K_FINAL, 2, src, dst, gr.br)
                   : two_pass_conv(grid(), ADMM_K_FINAL, 2, src, dst, gr.br);
    });
    if (rc) return rc;
    return ln.finish();
}

// ---- several branches in one grid ----------------------------------------------------------------------------
int launch_forward_multi(const Call& c, const MultiLayout& L) {
    int rc = ADMM_OK;
    unsigned char* ws = static_cast<unsigned char*>(c.workspace);
    hipStream_t s = reinterpret_cast<hipStream_t>(c.stream);
    Launcher ln{s, g_prof.on, {}};
    const float* y = c.y;
    float* x_out = c.x_out;
    const int M = c.M, N = c.N, nbr = c.nbranch, maxit = c.maxit, flags = c.flags;
    const size_t planes = c.grid_planes();
    const MultiView v = view(ws, L);
    for (int i = 0; i < nbr; ++i) {
        float* Ct = at<float>(ws, L.C + (size_t)i * multi_C_bytes());
        void* F = ws + L.F + (size_t)i * multi_F_bytes();
        const admm::ScalarSrc sc{c.lam_b[i], c.rho_b[i], 0.f, 0.f};
        rc = ln.run(ADMM_K_SETUP, [&] {
            const size_t lds = (size_t)(M + N) * 16;
            const int nb = (int)(((size_t)(M / 2 + 1) * N + kThreads - 1) / kThreads);
            set_lds(admm::setup_kernel, lds);
            hipLaunchKernelGGL(admm::setup_kernel, dim3(nb < 1024 ? nb : 1024), dim3(kThreads), lds, s, v.twM, v.twN, Ct,
                               (float2*)nullptr, (const float*)nullptr, 0, 0, M, N, sc, v.prm + 4 * i, (double2*)nullptr);
        });
        if (rc) return rc;
        if (L.two_pass) continue;   // the 2-pass kernels read Ct itself
        rc = ln.run(ADMM_K_SETUP, [&] { return admm::plane::launch_tables(Ct, nullptr, F, s); });
        if (rc) return rc;
    }
    if (maxit == 0) {
        hipError_t e = hipMemsetAsync(x_out, 0, planes * (size_t)M * N * 4, s);
        if (e != hipSuccess) return fail(ADMM_E_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
        return ln.finish();
    }
    const bool iso = (flags & ADMM_MULTI_ISO) != 0;
    const bool rec = (flags & ADMM_MULTI_RECORD) != 0, masks = rec && (flags & ADMM_REC_MASKS) != 0;
    if (L.two_pass) {
        // recording: s_it into slot it - 1 of traj, |s_it| (per branch) into slot it - 1 of nrm; otherwise the s
        // buffers sA / sbA in turn (isotropic: sA in place)
        Traj tr;
        tr.s = rec ? reinterpret_cast<float*>(v.traj) : nullptr;
        tr.nrm = rec && iso ? v.nrm : nullptr;
        float* sA = rec ? nullptr : at<float>(ws, L.sA);
        rc = two_pass_forward(two_pass_multi(ln, c, line_T(M, N), L), y, x_out, maxit, iso, tr, sA,
                              rec || iso ? sA : at<float>(ws, L.sbA));
        if (rc) return rc;
        return ln.finish();
    }
    const admm::plane::Branches br = multi_branches(c, multi_F_bytes());
    if (iso) {
        // each branch's batch norm over its own planes; recording: s_{k+1} into slot k, |s_{k+1}| too
        const size_t kE = (size_t)M * N / 2;
        const FusedIso f{ws + L.F, v.prm, planes, &br, reinterpret_cast<float4*>(rec ? v.traj : v.sln),
                         rec ? planes * kE : 0, rec ? reinterpret_cast<float2*>(v.nrm) : nullptr, nbr * kE,
                         reinterpret_cast<float2*>(v.fmap), reinterpret_cast<float2*>(v.qpart)};
        rc = fused_iso_forward(ln, f, y, x_out, false, v.hln, maxit);
        if (rc) return rc;
        return ln.finish();
    }
    rc = ln.run(ADMM_K_PLANE, [&] {
        return admm::plane::launch_plane(y, x_out, ws + L.F, false, v.hln, reinterpret_cast<float4*>(v.sln), v.prm, maxit,
                                         planes, s, rec && !masks ? reinterpret_cast<float4*>(v.traj) : nullptr, &br,
                                         masks ? reinterpret_cast<unsigned*>(v.traj) : nullptr);
    });
    if (rc) return rc;
    return ln.finish();
}

int launch_backward_multi(const Call& c, const Grads& g, const MultiLayout& L) {
    int rc = ADMM_OK;
    unsigned char* ws = static_cast<unsigned char*>(c.workspace);
    hipStream_t s = reinterpret_cast<hipStream_t>(c.stream);
    Launcher ln{s, g_prof.on, {}};
    const float *x_bar = g.x_bar, *x_out = c.x_out;
    float *y_bar = g.y_bar, *lambda_bar = g.lambda_bar, *rho_bar = g.rho_bar;
    const int M = c.M, N = c.N, nbr = c.nbranch, K = c.maxit, flags = c.flags;
    const size_t planes = c.grid_planes(), ppb = c.planes(), MN = (size_t)M * N;
    if (K == 0) {
        if (y_bar) HIPCHK(hipMemsetAsync(y_bar, 0, ppb * MN * 4, s));
        if (lambda_bar) HIPCHK(hipMemsetAsync(lambda_bar, 0, (size_t)nbr * 4, s));
        if (rho_bar) HIPCHK(hipMemsetAsync(rho_bar, 0, (size_t)nbr * 4, s));
        return ln.finish();
    }
    const MultiView v = view(ws, L);
    const bool iso = (flags & ADMM_MULTI_ISO) != 0;
    if (L.two_pass) {
        const SweepBufs b{reinterpret_cast<const float*>(v.traj), iso ? v.nrm : nullptr, nullptr, nullptr,
                          {at<float>(ws, L.sbA), at<float>(ws, L.sbB)}, y_bar ? at<float>(ws, L.vsum) : nullptr,
                          at<float>(ws, L.wbar), v.rmap, at<float>(ws, L.Rpart), v.part, rho_bar ? x_out : nullptr};
        // k = 1 launches no ISO_ADJ_R: its partial rows must read as zero
        if (iso) HIPCHK(hipMemsetAsync(v.part, 0, (size_t)nbr * L.pbs * 8, s));
        if (b.vsum) HIPCHK(hipMemsetAsync(b.vsum, 0, planes * MN * 4, s));
        rc = two_pass_reverse(two_pass_multi(ln, c, bwd_line_T(M, N, iso), L), b, x_bar, K, iso, false);
        if (rc) return rc;
        rc = branch_grads(ln, v, L.pbs, K * L.rows_b, lambda_bar, rho_bar, b.vsum, y_bar, ppb * MN, nbr);
        if (rc) return rc;
        return ln.finish();
    }
    const admm::plane::Branches br = multi_branches(c, multi_F_bytes());
    // each branch's Vsum in the natural layout (per grid plane): the forward's H^T y copies are dead
    float* vout = y_bar ? reinterpret_cast<float*>(v.hln) : nullptr;
    if (iso) {
        // vbar in the forward's dead s state, Vsum lane-native in vsl, R partials in the q partial slots
        const size_t kE = MN / 2, rows = multi_iso_rows(K);
        HIPCHK(hipMemsetAsync(v.part, 0, (size_t)nbr * rows * 16, s));
        const FusedIso f{ws + L.F, v.prm, planes, &br, reinterpret_cast<float4*>(v.traj), planes * kE,
                         reinterpret_cast<float2*>(v.nrm), nbr * kE, nullptr, reinterpret_cast<float2*>(v.qpart)};
        rc = fused_iso_reverse(ln, f, x_bar, reinterpret_cast<float2*>(v.sln), reinterpret_cast<float4*>(v.sbar),
                               reinterpret_cast<float2*>(v.rmap), reinterpret_cast<float2*>(v.vsl), vout, v.part, rows * 2, K);
        if (rc) return rc;
        rc = branch_grads(ln, v, rows * 2, (int)rows, lambda_bar, rho_bar, vout, y_bar, ppb * MN, nbr);
        if (rc) return rc;
        return ln.finish();
    }
    // D x_K in the forward's s state, which is dead
    rc = fused_reverse(ln, x_bar, ws + L.F, v.traj, (flags & ADMM_REC_MASKS) != 0, rho_bar ? x_out : nullptr,
                       reinterpret_cast<float4*>(v.sln), reinterpret_cast<float4*>(v.sbar),
                       reinterpret_cast<float2*>(v.vsl), vout, v.part, v.prm, K, planes, &br);
    if (rc) return rc;
    rc = branch_grads(ln, v, 2 * ppb, (int)ppb, lambda_bar, rho_bar, vout, y_bar, ppb * MN, nbr);
    if (rc) return rc;
    return ln.finish();
}

#undef HIPCHK

// ---- the grouped adjoint's instantiations of the 2-pass kernels (last: see "template dispatch" above) ----
int launch_column_grouped_adj(int N, int mode, dim3 g, size_t lds, hipStream_t s, const float2* src, float2* dst,
                              const float* C, const float2* G, const float2* twN, int L, int KB, float cs, float2* vsave,
                              double* Qp, const Branches& br, float2* yh) {
    switch (mode) {
        case 0: return launch_column_t<0, false, false, YH_NONE, true>(N, g, lds, s, src, dst, C, G, twN, L, KB, cs, vsave, Qp, br);
        case 2: return launch_column_t<2, false, false, YH_NONE, true>(N, g, lds, s, src, dst, C, G, twN, L, KB, cs, vsave, Qp, br);
        case 4: return launch_column_t<0, false, true, YH_NONE, true>(N, g, lds, s, src, dst, C, G, twN, L, KB, cs, vsave, Qp, br);
        case 7: return launch_column_t<0, true, false, YH_ADD, true>(N, g, lds, s, src, dst, C, G, twN, L, KB, cs, vsave, Qp, br, yh);
    }
    return -1;
}

int launch_line_adj_grouped(int L, int T, dim3 g, size_t lds, hipStream_t s, const float2* spec1, const float* sk1,
                            const float* sk, const float* xK, const float* sb_in, float* sb_out, float* vsum, float2* spec0,
                            double* part, const float2* twM, int N, const float* prm, int first_k, int last_k, bool ln,
                            const Branches& br) {
#define XG(l, t, lane)                                                                                               \
    if (L == l && T == t && ln == lane) {                                                                            \
        set_lds(line_adj_kernel<l, t, lane, true>, lds);                                                             \
        line_adj_kernel<l, t, lane, true><<<g, kThreads, lds, s>>>(spec1, sk1, sk, xK, sb_in, sb_out, vsum, spec0,   \
                                                                    part, twM, N, prm, first_k, last_k, br, 0);      \
        return 0;                                                                                                    \
    }
#define X(l, t) XG(l, t, false)
    ADMM_LT_CASES(X)
#undef X
    XG(128, 2, true) XG(128, 4, true) XG(128, 8, true) XG(128, 16, true)
#undef XG
    return -1;
}

// ---- resumable solve --------------------------------------------------------------------------------------------
// The forward on the planned path (fused, 2-pass or runtime-length, from s_0 or the zero state), then the end kernels.
// 2-pass and runtime-length: after K iterations the s buffers hold s_{K-1} (K = 1: the caller's s_0, or nothing) and, isotropic, fmap its factor map;
// s_K = D x_K + u_{K-1} goes to state_out -- or, wanted for the residuals only, to the s buffer that is free.  The
// residual norms need z_K: isotropic, one more norm step over s_K (its factor map in st.fmapK).
int launch_forward_state(const Call& c, const StateLayout& L, int path) {
    Launcher ln{reinterpret_cast<hipStream_t>(c.stream), g_prof.on, {}};
    hipStream_t s = ln.s;
    unsigned char* ws = static_cast<unsigned char*>(c.workspace);
    const StateIO& st = *c.st;
    const bool iso = c.iso != 0;
    const int M = c.M, N = c.N, K = c.maxit;
    const size_t planes = c.planes(), MN = (size_t)M * N;
    int rc = run_forward(ln, c, ws, L.f, Traj{}, path);
    const FwdView v = view(ws, L.f, c.kh > 0);
    if (!rc && (st.out || st.resid) && path == ADMM_PATH_FUSED) {
        // the fused kernel left s_{K-1} lane-native in s buffer 0 (K = 1: the imported s_0, or nothing); the residual
        // pass reads it in the natural layout from s buffer 1
        const float4* sln = K == 1 && !st.in ? nullptr : reinterpret_cast<const float4*>(v.s[0]);
        float* sK = st.out ? st.out : st.sK;
        float* s_prev = st.resid && sln ? v.s[1] : nullptr;
        rc = ln.run(ADMM_K_FINAL, [&] {
            return admm::plane::launch_state_end_lane(c.x_out, sln, sK, s_prev, v.prm, planes, s);
        });
        if (!rc && st.resid) rc = ln.run(ADMM_K_FINAL, [&] {
            return admm::st::launch_resid(sK, s_prev, nullptr, nullptr, false, st.rpart, st.resid, M, N, planes, v.prm, s);
        });
    } else if (!rc && (st.out || st.resid)) {
        // fwd_slots: iteration K - 1 wrote s_{K-1} to buffer 0 when K - 1 is odd or the prox isotropic (in place)
        const float* s_prev = K == 1 ? st.in : (iso || ((K - 1) & 1)) ? v.s[0] : v.s[1];
        float* sK = st.out ? st.out : s_prev == v.s[0] ? v.s[1] : v.s[0];
        rc = ln.run(ADMM_K_FINAL, [&] {
            return admm::st::launch_end(c.x_out, s_prev, v.fmap, iso, sK, M, N, planes, v.prm, s);
        });
        if (!rc && st.resid) {
            if (iso) {
                const int ng = iso_ngroups(planes);
                rc = ln.run(ADMM_K_NORM, [&] { return admm::st::launch_sq(sK, v.part, MN, planes, iso_group(planes), ng, s); });
                if (!rc) rc = iso_norm_step(ln, v.part, st.fmapK, ng, MN, v.prm, nullptr, nullptr);
            }
            if (!rc) rc = ln.run(ADMM_K_FINAL, [&] {
                return admm::st::launch_resid(sK, s_prev, st.fmapK, v.fmap, iso, st.rpart, st.resid, M, N, planes, v.prm, s);
            });
        }
    }
    const int rc2 = ln.finish();
    return rc ? rc : rc2;
}

}  // namespace admm_capi

// ---- the per-plane isotropic mode (ADMM_ISO_PLANE): its kernels and their instantiations, last of all ----
#include "admm_plane_bt.hip"

namespace admm_capi {

int launch_line_bt(int L, int T, dim3 g, size_t lds, hipStream_t s, const float2* spec1, float2* spec0, const float* so,
                   float* sn, const float2* twM, int N, const float* prm, int sz, int nt, const Branches& br) {
    // every (L, T, threads) launch_line dispatches, single (GRP = false) and grouped
#define X4(l, t, n, grp)                                                                                          \
    if (L == l && T == t && nt == n && (br.nbr == 0) == grp) {                                                    \
        set_lds(line_bt_kernel<l, t, n, grp>, lds);                                                               \
        line_bt_kernel<l, t, n, grp><<<g, n, lds, s>>>(spec1, spec0, so, sn, nullptr, twM, N, prm, sz, br);       \
        return 0;                                                                                                 \
    }
#define X3(l, t, n) X4(l, t, n, false) X4(l, t, n, true)
#define X(l, t) X3(l, t, kThreads)
    X3(256, 8, 512) X3(256, 16, 1024) X3(256, 4, 512) X3(256, 8, 1024)
    ADMM_LT_CASES(X)
#undef X
#undef X3
#undef X4
    return -1;
}

int launch_line_adj_bt(int L, int T, dim3 g, size_t lds, hipStream_t s, const float2* spec1, const float* sk1,
                       const float* sk, const float* xK, const float* sb_in, float* sb_out, float* vsum, float2* spec0,
                       double* part, const float2* twM, int N, const float* prm, int first_k, int last_k,
                       const Branches& br) {
    if (br.nbr == 0) return -1;   // (the grouped adjoint has no per-plane isotropic form)
#define X(l, t)                                                                                                    \
    if (L == l && T == t) {                                                                                        \
        set_lds(line_adj_bt_kernel<l, t>, lds);                                                                    \
        line_adj_bt_kernel<l, t><<<g, kThreads, lds, s>>>(spec1, sk1, sk, xK, sb_in, sb_out, vsum, spec0, part,    \
                                                           twM, N, prm, first_k, last_k, br);                      \
        return 0;                                                                                                  \
    }
    ADMM_LT_CASES(X)
#undef X
    return -1;
}

int launch_gen_line_upd_bt(dim3 g, size_t lds, hipStream_t s, const float* x, const float* so, float* sn, float2* spec,
                           const float2* twM, const admm::gen::FPlan& pM, int N, int T, const float* prm, int first,
                           const Branches& br) {
    set_lds(admm::gen::line_upd_bt_kernel, lds);
    hipLaunchKernelGGL(admm::gen::line_upd_bt_kernel, g, dim3(256), lds, s, x, so, sn, (const float*)nullptr, spec, twM, pM,
                       N, T, prm, first, br);
    return 0;
}

int launch_gen_line_adj_bt(dim3 g, size_t lds, hipStream_t s, const float* vb, const float* sk1, const float* sk,
                           const float* xK, const float* sb_in, float* sb_out, float* vsum, float2* spec, double* part,
                           const float2* twM, const admm::gen::FPlan& pM, int N, int T, const float* prm,
                           const Branches& br) {
    set_lds(admm::gen::line_adj_bt_kernel, lds);
    hipLaunchKernelGGL(admm::gen::line_adj_bt_kernel, g, dim3(256), lds, s, vb, sk1, sk, xK, sb_in, sb_out, vsum, spec, part,
                       twM, pM, N, T, prm, br);
    return 0;
}

}  // namespace admm_capi
