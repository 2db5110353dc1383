// admm_capi.hip -- extern "C" boundary (include/admm_deconv.h) for the ADMM TV-deconvolution
// solve on MI355X.  Replaces tvd_fft / tvd_fft_gpu (/root/reference/src/ops/ops.jl:99-188).
//
// This translation unit is the ABI: it validates every call, carves and queries the caller's workspace,
// keeps the recordings registry (a replay must match its recording) and the profiler, and hands the call
// to the launch sequencing (admm_launch.hip) with the plan of the path table (admm_paths.hip).  Nothing is
// allocated and nothing synchronises unless the optional profiler is on.
// Each entry point fills a Call (and an adjoint a Grads, capi_internal.hpp) once -- the shape-only size queries with the
// fields they have -- and plans it through forward_in / adjoint_in (admm_paths.hip), so a query, a workspace size and a
// solve of the same call take the same plan.  Below that there is one validation (check_call), one workspace carver
// (Carver; take_group_tables for the per-group table blocks), one registry (rec_store / rec_forget / rec_take: nothing
// else locks it) and one adjoint (run_backward) for the single and the grouped family.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <mutex>
#include <unordered_map>
#include <string>

#include "capi_internal.hpp"
#include "state_api.hpp"

namespace admm {
// admm_clamp_backward_f32: four elements per thread (16-B accesses when the three pointers allow), grid-strided
__global__ __launch_bounds__(256) void clamp_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                        float* dx, size_t n, float lo, float hi) {
    const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(dx)) &
                      15) == 0;
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * 256 * 4) {
        if (vec && i + 4 <= n) {
            const float4 a = *reinterpret_cast<const float4*>(x + i);
            const float4 g = *reinterpret_cast<const float4*>(dy + i);
            float4 r;
            r.x = (a.x >= lo && a.x <= hi) ? g.x : 0.0f;
            r.y = (a.y >= lo && a.y <= hi) ? g.y : 0.0f;
            r.z = (a.z >= lo && a.z <= hi) ? g.z : 0.0f;
            r.w = (a.w >= lo && a.w <= hi) ? g.w : 0.0f;
            *reinterpret_cast<float4*>(dx + i) = r;
        } else {
            for (size_t j = i; j < i + 4 && j < n; ++j) dx[j] = (x[j] >= lo && x[j] <= hi) ? dy[j] : 0.0f;
        }
    }
}
}  // namespace admm

namespace admm_capi {

thread_local std::string g_err;
Prof g_prof;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

}  // namespace admm_capi

namespace admm_internal {
// error reporting for the other translation units of the library (metrics_capi.hip)
int fail_msg(int code, const char* msg) {
    admm_capi::g_err = msg;
    return code;
}
}  // namespace admm_internal

namespace admm_capi {

int check_shape(int M, int N, int P, int B, int kh, int kw, int iso) {
    if (P < 1 || B < 1 || M < 1 || N < 1) return fail(ADMM_E_INVALID, "sizes must be positive (M=%d N=%d P=%d B=%d)", M, N, P, B);
    if (kh < 0 || kw < 0 || ((kh == 0) != (kw == 0)))
        return fail(ADMM_E_INVALID, "PSF size must be both zero (empty PSF) or both positive (kh=%d kw=%d)", kh, kw);
    // M, N >= 2 as in the reference (ops.jl:32-33 index the second row / column of the D stencils)
    if (M < 2 || N < 2 || M > kGenMax || N > kGenMax)
        return fail(ADMM_E_UNSUPPORTED, "this build supports 2<=M<=%d, 2<=N<=%d (got M=%d N=%d)", kGenMax, kGenMax, M, N);
    if (kh > M || kw > N)
        return fail(ADMM_E_UNSUPPORTED, "PSF %dx%d larger than the image (kh<=M, kw<=N required, as pad_constant in ops.jl:25)", kh, kw);
    if (iso_batch(iso) && (size_t)P * B > 65535)
        return fail(ADMM_E_UNSUPPORTED, "isotropic prox couples the batch: at most 65535 planes per call");
    return ADMM_OK;
}

int no_plane_mode(int iso, const char* who) {
    if (!iso_plane(iso)) return ADMM_OK;
    return fail(ADMM_E_UNSUPPORTED, "%s has no per-plane isotropic form (iso = ADMM_ISO_PLANE)", who);
}

}  // namespace admm_capi

namespace admm_capi {

int check_ws(void* workspace, size_t have, size_t need) {
    if (!workspace || have < need) return fail(ADMM_E_WORKSPACE, "workspace too small: need %zu bytes, got %zu", need, have);
    if ((reinterpret_cast<uintptr_t>(workspace) & 255) != 0) return fail(ADMM_E_WORKSPACE, "workspace must be 256-byte aligned");
    return ADMM_OK;
}

BwdLayout make_bwd_layout(int M, int N, size_t planes, int kh, int kw, int maxit, bool want_h, bool iso,
                          bool masks) {
    BwdLayout b{};
    const BwdHead hd = bwd_head(M, N, planes, kh, maxit, want_h, iso, masks);
    b.f = hd.f;
    b.traj_s = hd.traj_s, b.traj_v = hd.traj_v, b.sig = hd.sig, b.sbA = hd.sbA, b.sbB = hd.sbB, b.vsum = hd.vsum;
    b.traj_n = hd.traj_n;
    Carver cv{hd.end};
    const size_t MN = (size_t)M * N;
    const int K = maxit < 1 ? 1 : maxit;
    const bool gen = generic_shape(M, N);
    const int T = gen ? gen_T(M, N) : bwd_line_T(M, N, iso);
    const bool hq = want_h && kh > 0;
    if (iso) {
        const size_t ng = iso_ngroups(planes);
        b.wbar = cv.take(planes * MN * 4);   // vbar_k handed from ISO_ADJ_A to ISO_ADJ_B
        b.Rmap = cv.take(MN * 4);
        b.Rpart = cv.take(ng * MN * 4);
        b.nblk_isoA = (int)(ng * gen_nb(N, T));
        b.nblk_isoR = kIsoAdjRBlocks;
        b.nblk_line = b.nblk_isoA + b.nblk_isoR;
        if (b.nblk_line < 512) b.nblk_line = 512;   // the fused sweep's 512 tau_bar rows per step (plane_iso.hip)
    } else {
        b.nblk_line = (int)(planes * gen_nb(N, T));
    }
    b.rpart = cv.take((size_t)K * b.nblk_line * 2 * 8);
    b.Qp = hq ? cv.take(planes * (size_t)(M / 2 + 1) * N * 8) : 0;   // fp64 accumulators
    b.Q = hq ? cv.take((size_t)(M / 2 + 1) * N * 8) : 0;
    b.TY = 1;   // h_bar correlation tile: the largest of 8, 4, 2, 1 lines dividing N
    for (int t = 8; t > 1; t >>= 1)
        if (N % t == 0) {
            b.TY = t;
            break;
        }
    b.nblk_corr = (int)(planes * (N / b.TY));
    b.hpart = kh > 0 ? cv.take((size_t)b.nblk_corr * kh * kw * 8) : 0;
    b.hcorr = kh > 0 ? cv.take((size_t)kh * kw * 8) : 0;
    b.hA = hq ? cv.take((size_t)kh * kw * 8) : 0;
    b.rt = cv.take(2 * 8);
    b.rtmp = cv.take((size_t)kRedParts * (kh * kw > 2 ? kh * kw : 2) * 8);
    b.total = cv.off;
    return b;
}

// ---- recordings: the path a forward-with-trajectory took, checked by its replay ----------------
// A recording lives in the caller's workspace; its replay must run the reverse sweep that matches the
// trajectory's layout (lane-native for the fused kernel, natural for the 2-pass and runtime-length
// paths) and the tile choices the workspace layout was sized with.  The host keeps one tag per
// recorded workspace; a replay whose arguments or library options differ from the recording's, or
// whose workspace holds no recording, fails with ADMM_E_INVALID instead of reading a foreign layout.
struct RecTag {
    int M, N, P, B, kh, kw, iso, maxit, want_h;
    int opts[ADMM_OPT_COUNT];
    // host-value lambda / rho of the recording (0, 0 for device-resident scalars, which the host cannot
    // read without a synchronisation): a replay with other host values is refused
    float lam, rho;
    int dev_scalars;
    int masks;   // the trajectory holds ST mask bytes (ADMM_REC_MASKS): no rho_bar
    int nbr;     // branches of a multi-branch recording (1: a single solve)
    int sharded; // recorded with a batch reducer: sharded calls plan without the plane-count rule, so a replay
                 // with (or without) one must match or it could plan another sweep than the trajectory's layout
    int grouped, gb, gp, nparam;   // a grouped recording (admm_tvd_forward_grouped_record_dev_f32) and its grouping
    bool operator==(const RecTag& o) const { return std::memcmp(this, &o, sizeof(RecTag)) == 0; }
};

// the tag of a call: a single solve's has nbr = 1 and grouped = 0, a grouped call's its grouping, a multi-branch
// recording's its branch count (every branch's scalars are device-resident: a replay is not given them) -- no family
// replays another's recording
RecTag make_tag(const Call& c, bool want_h, bool masks) {
    RecTag t;
    std::memset(&t, 0, sizeof(t));
    t.M = c.M, t.N = c.N, t.P = c.P, t.B = c.B, t.kh = c.kh, t.kw = c.kw, t.maxit = c.maxit;
    t.iso = iso_plane(c.iso) ? ADMM_ISO_PLANE : c.iso != 0;   // the mode: no prox replays another's recording
    t.want_h = want_h, t.masks = masks;
    t.nbr = c.nbranch;
    t.dev_scalars = c.sc.lam != nullptr || c.kind == kMulti;
    if (!t.dev_scalars) t.lam = c.sc.lam_v, t.rho = c.sc.rho_v;
    for (int i = 0; i < ADMM_OPT_COUNT; ++i) t.opts[i] = opt(i);
    t.sharded = c.red != nullptr;
    t.grouped = c.grouped(), t.gb = c.gb, t.gp = c.gp, t.nparam = c.nparam;
    return t;
}

// The registry: these three functions alone lock g_rec_mu and touch g_rec.
std::mutex g_rec_mu;
std::unordered_map<const void*, RecTag> g_rec;
void rec_store(const void* ws, const RecTag& tag) {
    std::lock_guard<std::mutex> lk(g_rec_mu);
    g_rec[ws] = tag;
}
void rec_forget(const void* ws) {
    std::lock_guard<std::mutex> lk(g_rec_mu);
    g_rec.erase(ws);
}
// A replay, under one lock acquisition: `match` is handed the tag recorded for ws (null: none), rebuilds from it the
// tag this replay must find and compares; the recording is consumed when it returns ADMM_OK, and kept otherwise.
template <typename Match>
int rec_take(const void* ws, Match&& match) {
    std::lock_guard<std::mutex> lk(g_rec_mu);
    const auto it = g_rec.find(ws);
    const int rc = match(it == g_rec.end() ? nullptr : &it->second);
    if (rc == ADMM_OK && it != g_rec.end()) g_rec.erase(it);
    return rc;
}

// a single solve's lambda and rho: host values, or device pointers read in-kernel
int check_lam_rho(float lambda, float rho) {
    if (!std::isfinite(lambda) || !std::isfinite(rho)) return fail(ADMM_E_INVALID, "lambda and rho must be finite");
    return ADMM_OK;
}
int check_dev_scalars(const float* lambda, const float* rho) {
    if (!lambda || !rho) return fail(ADMM_E_INVALID, "lambda and rho must be device pointers");
    return ADMM_OK;
}
admm::ScalarSrc host_sc(float lambda, float rho) { return admm::ScalarSrc{nullptr, nullptr, lambda, rho}; }
admm::ScalarSrc dev_sc(const float* lambda, const float* rho) { return admm::ScalarSrc{lambda, rho, 0.f, 0.f}; }

// Library streams of the MALL-resident schedule: created once per device, never destroyed (non-blocking; the
// forward orders them against the caller's stream with events).
hipStream_t lib_stream(int i) {
    static std::mutex mu;
    static std::vector<std::vector<hipStream_t>> pool;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    if ((int)pool.size() <= dev) pool.resize(dev + 1);
    auto& v = pool[dev];
    while ((int)v.size() <= i) {
        hipStream_t st = nullptr;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return nullptr;
        v.push_back(st);
    }
    return v[i];
}

// A plain forward as it will run: its path, its chunk schedule, the layout of one chunk and the workspace it needs (one
// chunk layout, or one per stream of the MALL-resident schedule).
struct FwdSetup {
    PathPlan pl;
    ChunkPlan cp;
    Layout lay;
    size_t bytes;
};
FwdSetup forward_setup(const Call& c) {
    const PathIn q = forward_in(c);
    FwdSetup f;
    f.pl = plan_paths(q);
    f.cp = forward_chunks(q, f.pl, c.planes());   // an isotropic batch is one chunk
    f.lay = make_layout(c.M, c.N, f.cp.chunk, c.kh > 0, q.iso);
    f.bytes = f.cp.streams > 1 ? (size_t)f.cp.streams * align_up(f.lay.total) : f.lay.total;
    return f;
}

// ---- validation: one function for the single and the grouped family, forward (phases = 0) and adjoint ----
int check_common(const float* y, float* x, int maxit) {
    if (!y || !x) return fail(ADMM_E_INVALID, "y and x_out must be device pointers");
    if (maxit < 0) return fail(ADMM_E_INVALID, "maxit must be >= 0 (got %d)", maxit);
    if ((reinterpret_cast<uintptr_t>(y) & 15) || (reinterpret_cast<uintptr_t>(x) & 15))
        return fail(ADMM_E_INVALID, "y and x_out must be 16-byte aligned");
    return ADMM_OK;
}

// the grouping of a grouped call or workspace query, after its shape
int check_grouped(int M, int N, int P, int B, int gb, int gp, int kh, int kw, int iso) {
    int rc = check_shape(M, N, P, B, kh, kw, iso);
    if (rc) return rc;
    if ((gb != 1 && gb != B) || (gp != 1 && gp != P))
        return fail(ADMM_E_INVALID, "grouped solve: gb must be 1 or B, gp 1 or P (gb=%d gp=%d B=%d P=%d)", gb, gp, B, P);
    if ((size_t)P * B > kChunkPlanes)
        return fail(ADMM_E_UNSUPPORTED, "grouped solve: at most %zu planes per call", kChunkPlanes);
    return ADMM_OK;
}

// the sizes, flags and options of a multi-branch call or workspace query
int check_multi(int M, int N, int P, int B, int nbr, int maxit, int flags) {
    if (P < 1 || B < 1 || nbr < 1) return fail(ADMM_E_INVALID, "sizes must be positive (P=%d B=%d nbranch=%d)", P, B, nbr);
    if (maxit < 0) return fail(ADMM_E_INVALID, "maxit must be >= 0 (got %d)", maxit);
    if (flags & ~(ADMM_MULTI_RECORD | ADMM_REC_MASKS | ADMM_MULTI_ISO)) return fail(ADMM_E_INVALID, "unknown flags 0x%x", flags);
    if (M != kMultiM || N != kMultiN || !fused_enabled())
        return fail(ADMM_E_UNSUPPORTED, "the multi-branch solve is the fused 256 x 256 kernels (got %d x %d%s); "
                                        "solve the branches one by one", M, N, fused_enabled() ? "" : ", option FUSED = 0");
    if ((flags & ADMM_MULTI_ISO) && (flags & ADMM_MULTI_RECORD) && !fused_adj_enabled())
        return fail(ADMM_E_UNSUPPORTED, "an isotropic multi-branch recording needs the fused reverse sweep (option FUSED_ADJ)");
    if ((size_t)P * B * nbr > kChunkPlanes)
        return fail(ADMM_E_UNSUPPORTED, "at most %zu planes (nbranch * P * B) per multi-branch call", kChunkPlanes);
    return ADMM_OK;
}

// phases: 0 = plain forward, else the adjoint's (run_backward); g: the adjoint's gradients (phases & 2: x_bar is read).
// A grouped recording accepts ADMM_REC_MASKS without honouring it (the full trajectory is recorded, so rho_bar stays
// available) and refuses unknown flag bits; a single recording's flags only plan.  A multi-branch call: phases 0 its
// forward (recording or not), 2 the replay (its prox and masks flag are the recording's: c.flags is not checked).
int check_call(const Call& c, int phases, const Grads* g, int rec_flags = 0) {
    if (c.kind == kMulti) {
        int rc = check_multi(c.M, c.N, c.P, c.B, c.nbranch, c.maxit, phases ? 0 : c.flags);
        if (rc) return rc;
        if (phases) {
            if (!g->x_bar || !c.x_out || (reinterpret_cast<uintptr_t>(g->x_bar) & 15) ||
                (reinterpret_cast<uintptr_t>(c.x_out) & 15) || (reinterpret_cast<uintptr_t>(g->y_bar) & 15))
                return fail(ADMM_E_INVALID, "x_bar, x_out (and y_bar if given) must be 16-byte aligned device pointers");
            return ADMM_OK;
        }
        rc = check_common(c.y, c.x_out, c.maxit);
        if (rc) return rc;
        if (!c.lam_b || !c.rho_b) return fail(ADMM_E_INVALID, "lambda and rho must be host arrays of nbranch device pointers");
        for (int i = 0; i < c.nbranch; ++i)
            if (!c.lam_b[i] || !c.rho_b[i]) return fail(ADMM_E_INVALID, "lambda[%d] / rho[%d] must be device pointers", i, i);
        return ADMM_OK;
    }
    int rc = c.grouped() ? check_grouped(c.M, c.N, c.P, c.B, c.gb, c.gp, c.kh, c.kw, c.iso)
                         : check_shape(c.M, c.N, c.P, c.B, c.kh, c.kw, c.iso);
    if (rc) return rc;
    if (c.grouped()) {
        const char* who = phases ? "grouped adjoint" : "grouped solve";
        if (c.kh > 0 && !c.h) return fail(ADMM_E_INVALID, "%s: h is NULL with a %d x %d PSF", who, c.kh, c.kw);
        if (!c.sc.lam || !c.sc.rho) return fail(ADMM_E_INVALID, "%s: lambda and rho must be device pointers", who);
        if (c.nparam != 1 && c.nparam != c.groups())
            return fail(ADMM_E_INVALID, "%s: nparam must be 1 or the group count %d (got %d)", who, c.groups(), c.nparam);
        if (phases && no_plane_mode(c.iso, "the grouped adjoint")) return ADMM_E_UNSUPPORTED;
        if (iso_batch(c.iso) && c.nparam > 1)
            return fail(ADMM_E_UNSUPPORTED, "%s: the isotropic prox is one BT factor map per batch, so it takes one "
                                            "(lambda, rho) pair (nparam = 1), got %d", who, c.nparam);
        if (rec_flags & ~(ADMM_REC_HBAR | ADMM_REC_MASKS)) return fail(ADMM_E_INVALID, "%s: unknown rec_flags 0x%x", who, rec_flags);
    }
    rc = check_common(c.y, c.x_out, c.maxit);
    if (rc) return rc;
    if ((phases & 2) && (reinterpret_cast<uintptr_t>(g->y_bar) & 15))
        return fail(ADMM_E_INVALID, "y_bar must be a 16-byte aligned device pointer (or NULL: not needed)");
    if ((phases & 2) && (!g->x_bar || (reinterpret_cast<uintptr_t>(g->x_bar) & 15)))
        return fail(ADMM_E_INVALID, "x_bar must be a 16-byte aligned device pointer");
    if (phases && !c.grouped() && c.planes() > 65535)
        return fail(ADMM_E_UNSUPPORTED, "the adjoint takes at most 65535 planes per call (split the batch)");
    return ADMM_OK;
}

// a single solve's descriptor: h == NULL is "no PSF"; the reducer acts on the isotropic prox only
Call single_call(Call c) {
    if (c.h == nullptr) c.kh = c.kw = 0;
    c.red = (iso_batch(c.iso) && c.red && c.red->fn) ? c.red : nullptr;
    return c;
}

int forward_impl(const Call& c) {
    int rc = check_call(c, 0, nullptr);
    if (rc) return rc;
    const size_t planes = c.planes();
    const FwdSetup f = forward_setup(c);
    const size_t chunk = f.cp.chunk;
    rc = check_ws(c.workspace, c.workspace_bytes, f.bytes);
    if (rc) return rc;
    rec_forget(c.workspace);   // whatever was recorded there is overwritten now
    const hipStream_t s0 = reinterpret_cast<hipStream_t>(c.stream);
    unsigned char* ws = static_cast<unsigned char*>(c.workspace);
    if (f.cp.streams <= 1) {
        Launcher ln{s0, g_prof.on, {}};
        // the tables (twiddles, C / G, scalars) once: later chunks reuse them from the same workspace
        for (size_t p0 = 0; p0 < planes && rc == 0; p0 += chunk)
            rc = run_forward(ln, c, ws, f.lay, Traj{}, f.pl.fwd, p0 == 0, p0, std::min(chunk, planes - p0));
        int rc2 = ln.finish();
        return rc ? rc : rc2;
    }
    // MALL-resident schedule: chunk i on stream i mod n (the caller's stream and n - 1 library streams), each stream
    // with its own chunk workspace; fork and join through events on the caller's stream
    const int n = f.cp.streams;
    const size_t stride = align_up(f.lay.total);
    std::vector<Launcher> lns;
    lns.reserve(n);
    lns.push_back(Launcher{s0, g_prof.on, {}});
    hipEvent_t fork = nullptr;
    if (hipEventCreateWithFlags(&fork, hipEventDisableTiming) != hipSuccess || hipEventRecord(fork, s0) != hipSuccess)
        return fail(ADMM_E_HIP, "MALL schedule: fork event");
    for (int k = 1; k < n; ++k) {
        hipStream_t sk = lib_stream(k - 1);
        if (!sk || hipStreamWaitEvent(sk, fork, 0) != hipSuccess) {
            hipEventDestroy(fork);
            return fail(ADMM_E_HIP, "MALL schedule: library stream %d", k);
        }
        lns.push_back(Launcher{sk, g_prof.on, {}});
    }
    hipEventDestroy(fork);   // (released once the waits have consumed it)
    size_t i = 0;
    for (size_t p0 = 0; p0 < planes && rc == 0; p0 += chunk, ++i) {
        const int k = (int)(i % (size_t)n);
        // each stream's chunk workspace builds the tables with its first chunk (96 setup launches per c4 solve -> 4)
        rc = run_forward(lns[k], c, ws + (size_t)k * stride, f.lay, Traj{}, f.pl.fwd, i < (size_t)n, p0,
                         std::min(chunk, planes - p0));
    }
    // join: the caller's stream waits for every library stream (also after an error, so nothing is left running
    // against the caller's buffers unordered)
    for (int k = 1; k < n; ++k) {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess) {
            if (hipEventRecord(e, lns[k].s) != hipSuccess || hipStreamWaitEvent(s0, e, 0) != hipSuccess)
                rc = rc ? rc : fail(ADMM_E_HIP, "MALL schedule: join");
            hipEventDestroy(e);
        } else if (!rc) {
            rc = fail(ADMM_E_HIP, "MALL schedule: join event");
        }
    }
    for (auto& l : lns) {
        const int r2 = l.finish();
        if (!rc) rc = r2;
    }
    return rc;
}

// the per-group blocks of a grouped layout, behind cv: scalars, 2-pass C / G tables, lane-native tables; f's own
// slots are renamed to group 0's blocks
void take_group_tables(Carver& cv, Layout& f, int M, int N, size_t G, bool psf) {
    const size_t tab_f = group_tab_f(M, N);
    f.prm = cv.take(G * 16);
    f.C = cv.take(G * tab_f * 4);
    f.G = psf ? cv.take(G * tab_f * 8) : 0;
    f.F = fused_tables_shape(M, N) ? cv.take(G * admm::plane::grouped_tables_bytes()) : 0;
}

Layout make_grouped_layout(int M, int N, size_t planes, int groups, bool psf, bool iso) {
    Layout f = make_layout(M, N, planes, psf, iso);
    Carver cv{align_up(f.total)};
    take_group_tables(cv, f, M, N, (size_t)groups, psf);
    f.total = cv.off;
    return f;
}

int forward_grouped(const Call& c) {
    int rc = check_call(c, 0, nullptr);
    if (rc) return rc;
    const Layout lay = make_grouped_layout(c.M, c.N, c.planes(), c.groups(), c.kh > 0, iso_batch(c.iso));
    rc = check_ws(c.workspace, c.workspace_bytes, lay.total);
    if (rc) return rc;
    rec_forget(c.workspace);
    Launcher ln{reinterpret_cast<hipStream_t>(c.stream), g_prof.on, {}};
    rc = run_forward(ln, c, static_cast<unsigned char*>(c.workspace), lay, Traj{}, plan_paths(forward_in(c)).fwd);
    const int rc2 = ln.finish();
    return rc ? rc : rc2;
}

// ---- resumable solve ----
StateLayout make_state_layout(int M, int N, size_t planes, bool psf, bool iso) {
    StateLayout L{};
    L.f = make_layout(M, N, planes, psf, iso);
    Carver cv{align_up(L.f.total)};
    const size_t MN = (size_t)M * N;
    L.v0 = cv.take(planes * MN * 4);
    L.fmapK = iso ? cv.take(MN * 4) : 0;
    L.rpart = cv.take(planes * (size_t)admm::st::resid_blocks(MN, planes) * admm::st::kResidSums * 8);
    L.sK = fused_shape(M, N, iso) ? cv.take(planes * 2 * MN * 4) : 0;
    L.total = cv.off;
    return L;
}

int check_state_shape(int M, int N, int P, int B, int kh, int kw, int iso) {
    const int rc = check_shape(M, N, P, B, kh, kw, iso);
    if (rc) return rc;
    if ((size_t)P * B > kChunkPlanes) return fail(ADMM_E_UNSUPPORTED, "state call: at most %zu planes per call", kChunkPlanes);
    return ADMM_OK;
}

int forward_state(Call c, const float* state_in, float* state_out, float* resid_out) {
    if (no_plane_mode(c.iso, "the state call")) return ADMM_E_UNSUPPORTED;
    int rc = check_state_shape(c.M, c.N, c.P, c.B, c.kh, c.kw, c.iso);
    if (rc) return rc;
    if (c.kh > 0 && !c.h) return fail(ADMM_E_INVALID, "state call: h is NULL with a %d x %d PSF", c.kh, c.kw);
    rc = check_common(c.y, c.x_out, c.maxit);
    if (rc) return rc;
    if (c.maxit < 1)
        return fail(ADMM_E_INVALID, "state call: maxit must be >= 1 (x is not part of the state: no iteration, no x)");
    if (state_out && state_out == state_in) return fail(ADMM_E_INVALID, "state call: state_out must not be state_in");
    if ((reinterpret_cast<uintptr_t>(state_in) & 15) || (reinterpret_cast<uintptr_t>(state_out) & 15))
        return fail(ADMM_E_INVALID, "state call: state_in and state_out must be 16-byte aligned");
    const StateLayout L = make_state_layout(c.M, c.N, c.planes(), c.kh > 0, c.iso != 0);
    rc = check_ws(c.workspace, c.workspace_bytes, L.total);
    if (rc) return rc;
    rec_forget(c.workspace);
    unsigned char* ws = static_cast<unsigned char*>(c.workspace);
    const StateIO st{state_in, state_out, resid_out, reinterpret_cast<float*>(ws + L.v0),
                     c.iso ? reinterpret_cast<float*>(ws + L.fmapK) : nullptr, reinterpret_cast<double*>(ws + L.rpart),
                     L.sK ? reinterpret_cast<float*>(ws + L.sK) : nullptr};
    c.st = &st;
    return launch_forward_state(c, L, plan_paths(forward_in(c)).fwd);
}

BwdLayout make_grouped_bwd_layout(const Call& c, bool want_h) {
    const int M = c.M, N = c.N;
    const size_t planes = c.planes(), G = (size_t)c.groups(), ntaps = (size_t)c.kh * c.kw;
    const bool psf = c.kh > 0, hq = want_h && psf, iso = iso_batch(c.iso);
    BwdLayout b = make_bwd_layout(M, N, planes, c.kh, c.kw, c.maxit, want_h, iso);
    Carver cv{align_up(b.total)};
    take_group_tables(cv, b.f, M, N, G, psf);
    // per group: PSF spectrum, Q, the two h_bar terms, the (rho_bar, tau_bar) sums
    const size_t nq = (size_t)(M / 2 + 1) * N;
    b.sig = hq ? cv.take(G * nq * 16) : 0;
    b.Q = hq ? cv.take(G * nq * 8) : 0;
    b.hcorr = psf ? cv.take(G * ntaps * 8) : 0;
    b.hA = hq ? cv.take(G * ntaps * 8) : 0;
    b.rt = cv.take(G * 2 * 8);
    // parts of the group-segmented sums: one (lambda, rho) pair sums every plane's rows, G pairs a group's
    const int K = c.maxit < 1 ? 1 : c.maxit;
    const size_t ppg = planes / G;
    b.split_rt = iso ? 1 : group_split((long long)K * (b.nblk_line / (long long)planes) * (c.nparam > 1 ? ppg : planes));
    b.split_h = psf ? group_split((long long)(N / b.TY) * ppg) : 1;
    const size_t t_rt = (size_t)c.nparam * b.split_rt * 2, t_h = G * b.split_h * ntaps;
    b.gtmp = cv.take((t_rt > t_h ? t_rt : t_h) * 8);
    b.total = cv.off;
    return b;
}

// the adjoint workspace of a single or a grouped call planned as pl (mask bytes in place of s_k: anisotropic only)
BwdLayout adjoint_layout(const Call& c, const PathPlan& pl) {
    if (c.grouped()) return make_grouped_bwd_layout(c, pl.want_h);
    const bool iso = iso_batch(c.iso);
    return make_bwd_layout(c.M, c.N, c.planes(), c.kh, c.kw, c.maxit, pl.want_h, iso, pl.masks && !iso);
}

// The adjoint of a single or a grouped call.  phases: 1 = forward recording the trajectory into the workspace (writes
// x_out), 2 = reverse sweep from a recorded workspace (x_out = that forward's output), 3 = both.  rec_flags
// (ADMM_REC_*): phase 1 alone records the extra h_bar trajectory only when asked (phase 2 must then be given h_bar).
// A grouped call has no reducer form; its grouping, layouts and validation are the grouped forward's.
int run_backward(int phases, int rec_flags, const Call& c, const Grads& g) {
    int rc = check_call(c, phases, &g, rec_flags);
    if (rc) return rc;
    PathPlan plan;
    BwdLayout bl;
    RecTag tag;
    // plan, lay out, check the workspace, tag.  A replay (phase 2) is planned as the recording it replays was: masks
    // is the recording's flag (a replay whose options or arguments differ is rejected by its tag below).
    auto prepare = [&](bool masks) {
        plan = plan_paths(adjoint_in(c, phases, rec_flags, g, masks));
        bl = adjoint_layout(c, plan);
        tag = make_tag(c, plan.want_h, plan.masks);
        return check_ws(c.workspace, c.workspace_bytes, bl.total);
    };
    if (phases != 2) {
        rc = prepare(false);
        if (rc) return rc;
        if (phases == 1) rec_store(c.workspace, tag);
        else rec_forget(c.workspace);
        return launch_backward(phases, c, g, plan, bl);
    }
    rc = rec_take(c.workspace, [&](const RecTag* rec) -> int {
        const int r = prepare(rec && rec->masks);
        if (r) return r;
        if (!rec)
            return fail(ADMM_E_INVALID, "workspace holds no recording (%s first; a plain forward on the same workspace "
                                        "overwrites it)",
                        c.grouped() ? "admm_tvd_forward_grouped_record_dev_f32" : "admm_tvd_forward_record_*");
        if (!(*rec == tag))
            return c.grouped()
                       ? fail(ADMM_E_INVALID, "replay does not match its grouped recording (shape, grouping gb / gp / nparam, "
                                              "PSF, iso, maxit, h_bar request or library options changed between record and "
                                              "replay, or the recording is a single solve's)")
                       : fail(ADMM_E_INVALID, "replay does not match its recording (shape, PSF, iso, maxit, h_bar request, "
                                              "lambda / rho, library options or the batch reducer (sharded or not) changed "
                                              "between record and replay)");
        if (plan.masks && g.rho_bar)
            return fail(ADMM_E_INVALID, "recorded with ADMM_REC_MASKS (soft-threshold branches only / the fused isotropic "
                                        "trajectory): rho_bar cannot be formed from it; record without the flag to get rho_bar");
        return ADMM_OK;
    });
    if (rc) return rc;
    return launch_backward(phases, c, g, plan, bl);
}

size_t multi_C_bytes() { return align_up((size_t)(kMultiM / 2 + 1) * kMultiN * 4); }
size_t multi_F_bytes() { return align_up(admm::plane::tables_bytes()); }

// tau_bar partial rows of one branch's isotropic sweep: 512 per reverse step k = K .. 2 (iso_radj_kernel)
size_t multi_iso_rows(int K) { return (size_t)(K > 1 ? K - 1 : 1) * 512; }

// the workspace of a multi-branch call (c.flags: the forward's, or the recording's for its replay), for the grid it is
// planned on
MultiLayout make_multi_layout(const Call& c) {
    MultiLayout L{};
    Carver cv{0};
    const size_t MN = (size_t)kMultiM * kMultiN, planes = c.grid_planes();
    const int nbr = c.nbranch, flags = c.flags, K = c.maxit < 1 ? 1 : c.maxit;
    const bool rec = (flags & ADMM_MULTI_RECORD) != 0, iso = (flags & ADMM_MULTI_ISO) != 0;
    const bool masks = (flags & ADMM_REC_MASKS) != 0 && !iso;
    L.prm = cv.take((size_t)nbr * 16);
    L.twM = cv.take(kMultiM * 8);
    L.twN = cv.take(kMultiN * 8);
    L.C = cv.take((size_t)nbr * multi_C_bytes());
    const int fwd = plan_paths(forward_in(c)).fwd;
    L.two_pass = fwd == ADMM_PATH_2PASS || fwd == ADMM_PATH_2PASS_ISO;
    if (L.two_pass) {
        // the 2-pass kernels over every branch's planes (admm_launch.hip two_pass_multi)
        const size_t ppb = planes / (size_t)nbr;
        const int T = bwd_line_T(kMultiM, kMultiN, iso);
        if (iso) {
            L.G = iso_group(ppb);
            L.ngb = iso_ngroups(ppb);
            L.nblk_a = L.ngb * (kMultiN / T);
            L.rows_b = L.nblk_a + kIsoAdjRBlocks;
        } else {
            L.rows_b = (int)ppb * (kMultiN / T);
        }
        L.pbs = (size_t)K * L.rows_b * 2;
        L.spec0 = cv.take(planes * MN * 4);
        L.spec1 = cv.take(planes * MN * 4);
        L.hln = cv.take(planes * MN * 4);   // Y_h = F y per grid plane (H^T y in the spectral domain)
        if (iso) {
            L.fmap = cv.take((size_t)nbr * MN * 4);
            L.qpart = cv.take((size_t)nbr * L.ngb * MN * 4);
        }
        if (rec) {
            L.traj = cv.take((size_t)(K > 1 ? K - 1 : 1) * planes * MN * 8);
            L.sbA = cv.take(planes * MN * 8);
            L.sbB = cv.take(planes * MN * 8);
            L.vsum = cv.take(planes * MN * 4);
            L.part = cv.take((size_t)nbr * L.pbs * 8);
            L.rt = cv.take((size_t)nbr * 16);
            L.rtmp = cv.take((size_t)kRedParts * 2 * 8);
            if (iso) {
                L.nrm = cv.take((size_t)(K > 1 ? K - 1 : 1) * nbr * MN * 4);
                L.wbar = cv.take(planes * MN * 4);
                L.rmap = cv.take((size_t)nbr * MN * 4);
                L.Rpart = cv.take((size_t)nbr * L.ngb * MN * 4);
            }
        } else {
            L.sA = cv.take(planes * MN * 8);
            if (!iso) L.sbA = cv.take(planes * MN * 8);   // the anisotropic s ping-pong's second buffer
        }
        L.total = cv.off;
        return L;
    }
    L.F = cv.take((size_t)nbr * multi_F_bytes());
    L.hln = cv.take(admm::plane::hty_bytes(planes));   // lane-native H^T y at its skewed plane stride
    L.sln = cv.take(planes * MN * 8);
    if (rec) {
        L.traj = cv.take((size_t)(K > 1 ? K - 1 : 1) * planes * (masks ? MN / 2 : MN * 8));
        L.sbar = cv.take(planes * MN * 8);
        L.vsl = cv.take(planes * MN * 4);
        L.part = cv.take(iso ? (size_t)nbr * multi_iso_rows(K) * 16 : planes * 16);
        L.rt = cv.take((size_t)nbr * 16);
        L.rtmp = cv.take((size_t)kRedParts * 2 * 8);
    }
    if (iso) {
        L.fmap = cv.take((size_t)nbr * MN * 4);
        L.qpart = cv.take(planes * MN * 4);
        if (rec) {
            L.nrm = cv.take((size_t)(K > 1 ? K - 1 : 1) * nbr * MN * 4);
            L.rmap = cv.take((size_t)nbr * MN * 4);
        }
    }
    L.total = cv.off;
    return L;
}

// a multi-branch call's descriptor from the sizes and flags every entry of the family has: no PSF, the prox from flags
Call multi_call(int M, int N, int P, int B, int nbranch, int maxit, int flags) {
    Call c = shape_call(M, N, P, B, 0, 0, (flags & ADMM_MULTI_ISO) != 0, maxit);
    c.kind = kMulti, c.nbranch = nbranch, c.flags = flags;
    return c;
}

int forward_multi(const Call& c) {
    int rc = check_call(c, 0, nullptr);
    if (rc) return rc;
    const MultiLayout L = make_multi_layout(c);
    rc = check_ws(c.workspace, c.workspace_bytes, L.total);
    if (rc) return rc;
    // (masks: no rho_bar from the ST mask bits, nor from the isotropic recording)
    if (c.flags & ADMM_MULTI_RECORD) rec_store(c.workspace, make_tag(c, false, (c.flags & ADMM_REC_MASKS) != 0 || c.iso));
    else rec_forget(c.workspace);
    return launch_forward_multi(c, L);
}

// c.flags: none (a replay is not given them); the recording's prox and masks flag are taken from its tag
int backward_multi(Call c, const Grads& g) {
    int rc = check_call(c, 2, &g);
    if (rc) return rc;
    rc = rec_take(c.workspace, [&](const RecTag* rec) -> int {
        if (!rec || rec->nbr != c.nbranch)
            return fail(ADMM_E_INVALID, "workspace holds no multi-branch recording of %d branches "
                                        "(admm_tvd_forward_multi_dev_f32 with ADMM_MULTI_RECORD first)", c.nbranch);
        // the recording's prox and masks flag; everything else must be this call's
        c.iso = rec->iso;
        c.flags = ADMM_MULTI_RECORD | (rec->iso ? ADMM_MULTI_ISO : 0) | (rec->masks ? ADMM_REC_MASKS : 0);
        if (!(*rec == make_tag(c, false, rec->masks != 0)))
            return fail(ADMM_E_INVALID, "replay does not match its multi-branch recording (shape, maxit or library "
                                        "options changed)");
        if (rec->masks && g.rho_bar)
            return fail(ADMM_E_INVALID, "recorded with ADMM_REC_MASKS (soft-threshold branches only) or ADMM_MULTI_ISO: "
                                        "rho_bar cannot be formed from it");
        return ADMM_OK;
    });
    if (rc) return rc;
    const MultiLayout L = make_multi_layout(c);
    rc = check_ws(c.workspace, c.workspace_bytes, L.total);
    if (rc) return rc;
    return launch_backward_multi(c, g, L);
}

}  // namespace admm_capi

using namespace admm_capi;

extern "C" {

int admm_abi_version(void) { return ADMM_ABI_VERSION; }

int admm_iso_plane_supported(void) { return 1; }

const char* admm_last_error(void) { return g_err.c_str(); }

int admm_tvd_workspace_bytes(int M, int N, int P, int B, int kh, int kw, int iso, size_t* out_bytes) {
    if (!out_bytes) return fail(ADMM_E_INVALID, "out_bytes is NULL");
    int rc = check_shape(M, N, P, B, kh, kw, iso);
    if (rc) return rc;
    *out_bytes = forward_setup(shape_call(M, N, P, B, kh, kw, iso)).bytes;
    return ADMM_OK;
}

// The single-solve entry points: scalars checked, then Call / Grads filled in once.
#define ADMM_SINGLE(sc, x, red) \
    single_call(Call{y, x, M, N, P, B, h, kh, kw, sc, iso, maxit, workspace, workspace_bytes, stream, red})

int admm_tvd_forward_f32(const float* y, float* x_out, int M, int N, int P, int B, const float* h, int kh, int kw,
                         float lambda, float rho, int iso, int maxit, void* workspace, size_t workspace_bytes,
                         void* stream) {
    return admm_tvd_forward_sharded_f32(y, x_out, M, N, P, B, h, kh, kw, lambda, rho, iso, maxit, workspace,
                                        workspace_bytes, stream, nullptr);
}

int admm_tvd_forward_sharded_f32(const float* y, float* x_out, int M, int N, int P, int B, const float* h, int kh,
                                 int kw, float lambda, float rho, int iso, int maxit, void* workspace,
                                 size_t workspace_bytes, void* stream, const admm_batch_reducer* reducer) {
    const int rc = check_lam_rho(lambda, rho);
    return rc ? rc : forward_impl(ADMM_SINGLE(host_sc(lambda, rho), x_out, reducer));
}

int admm_tvd_forward_dev_f32(const float* y, float* x_out, int M, int N, int P, int B, const float* h, int kh, int kw,
                             const float* lambda, const float* rho, int iso, int maxit, void* workspace,
                             size_t workspace_bytes, void* stream, const admm_batch_reducer* reducer) {
    const int rc = check_dev_scalars(lambda, rho);
    return rc ? rc : forward_impl(ADMM_SINGLE(dev_sc(lambda, rho), x_out, reducer));
}

int admm_tvd_backward_workspace_bytes(int M, int N, int P, int B, int kh, int kw, int iso, int maxit, int want_hbar,
                                      size_t* out_bytes) {
    if (!out_bytes) return fail(ADMM_E_INVALID, "out_bytes is NULL");
    int rc = check_shape(M, N, P, B, kh, kw, iso);
    if (rc) return rc;
    if (maxit < 0) return fail(ADMM_E_INVALID, "maxit must be >= 0");
    if ((size_t)P * B > 65535) return fail(ADMM_E_UNSUPPORTED, "the adjoint takes at most 65535 planes per call (split the batch)");
    const Call c = shape_call(M, N, P, B, kh, kw, iso, maxit);
    *out_bytes = adjoint_layout(c, plan_paths(adjoint_in(c, 1, want_hbar, Grads{}))).total;
    return ADMM_OK;
}

int admm_tvd_backward_f32(const float* y, const float* x_bar, float* y_bar, float* h_bar, float* lambda_bar,
                          float* rho_bar, int M, int N, int P, int B, const float* h, int kh, int kw, float lambda,
                          float rho, int iso, int maxit, float* x_out, void* workspace, size_t workspace_bytes,
                          void* stream) {
    return admm_tvd_backward_sharded_f32(y, x_bar, y_bar, h_bar, lambda_bar, rho_bar, M, N, P, B, h, kh, kw, lambda,
                                         rho, iso, maxit, x_out, workspace, workspace_bytes, stream, nullptr);
}

int admm_tvd_backward_sharded_f32(const float* y, const float* x_bar, float* y_bar, float* h_bar, float* lambda_bar,
                                  float* rho_bar, int M, int N, int P, int B, const float* h, int kh, int kw,
                                  float lambda, float rho, int iso, int maxit, float* x_out, void* workspace,
                                  size_t workspace_bytes, void* stream, const admm_batch_reducer* reducer) {
    const int rc = check_lam_rho(lambda, rho);
    return rc ? rc : run_backward(3, 0, ADMM_SINGLE(host_sc(lambda, rho), x_out, reducer),
                                   Grads{x_bar, y_bar, h_bar, lambda_bar, rho_bar});
}

int admm_tvd_backward_dev_f32(const float* y, const float* x_bar, float* y_bar, float* h_bar, float* lambda_bar,
                              float* rho_bar, int M, int N, int P, int B, const float* h, int kh, int kw,
                              const float* lambda, const float* rho, int iso, int maxit, float* x_out, void* workspace,
                              size_t workspace_bytes, void* stream, const admm_batch_reducer* reducer) {
    const int rc = check_dev_scalars(lambda, rho);
    return rc ? rc : run_backward(3, 0, ADMM_SINGLE(dev_sc(lambda, rho), x_out, reducer),
                                   Grads{x_bar, y_bar, h_bar, lambda_bar, rho_bar});
}

int admm_tvd_forward_record_f32(const float* y, float* x_out, int M, int N, int P, int B, const float* h, int kh,
                                int kw, float lambda, float rho, int iso, int maxit, int want_hbar, void* workspace,
                                size_t workspace_bytes, void* stream, const admm_batch_reducer* reducer) {
    const int rc = check_lam_rho(lambda, rho);
    return rc ? rc : run_backward(1, want_hbar, ADMM_SINGLE(host_sc(lambda, rho), x_out, reducer), Grads{});
}

int admm_tvd_forward_record_dev_f32(const float* y, float* x_out, int M, int N, int P, int B, const float* h, int kh,
                                    int kw, const float* lambda, const float* rho, int iso, int maxit, int want_hbar,
                                    void* workspace, size_t workspace_bytes, void* stream,
                                    const admm_batch_reducer* reducer) {
    const int rc = check_dev_scalars(lambda, rho);
    return rc ? rc : run_backward(1, want_hbar, ADMM_SINGLE(dev_sc(lambda, rho), x_out, reducer), Grads{});
}

// (a replay reads x_out, the recorded forward's output)
int admm_tvd_backward_recorded_f32(const float* y, const float* x_bar, float* y_bar, float* h_bar, float* lambda_bar,
                                   float* rho_bar, int M, int N, int P, int B, const float* h, int kh, int kw,
                                   float lambda, float rho, int iso, int maxit, const float* x_out, void* workspace,
                                   size_t workspace_bytes, void* stream, const admm_batch_reducer* reducer) {
    const int rc = check_lam_rho(lambda, rho);
    return rc ? rc : run_backward(2, 0, ADMM_SINGLE(host_sc(lambda, rho), const_cast<float*>(x_out), reducer),
                                   Grads{x_bar, y_bar, h_bar, lambda_bar, rho_bar});
}

int admm_tvd_backward_recorded_dev_f32(const float* y, const float* x_bar, float* y_bar, float* h_bar,
                                       float* lambda_bar, float* rho_bar, int M, int N, int P, int B, const float* h,
                                       int kh, int kw, const float* lambda, const float* rho, int iso, int maxit,
                                       const float* x_out, void* workspace, size_t workspace_bytes, void* stream,
                                       const admm_batch_reducer* reducer) {
    const int rc = check_dev_scalars(lambda, rho);
    return rc ? rc : run_backward(2, 0, ADMM_SINGLE(dev_sc(lambda, rho), const_cast<float*>(x_out), reducer),
                                   Grads{x_bar, y_bar, h_bar, lambda_bar, rho_bar});
}
#undef ADMM_SINGLE

int admm_profile_enable(int on) {
    g_prof.on = on != 0;
    return ADMM_OK;
}

int admm_profile_reset(void) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    for (int i = 0; i < ADMM_K_COUNT; ++i) {
        g_prof.ms[i] = 0.0;
        g_prof.n[i] = 0;
    }
    return ADMM_OK;
}

int admm_profile_get(int kernel_class, double* total_ms, long long* launches) {
    if (kernel_class < 0 || kernel_class >= ADMM_K_COUNT || !total_ms || !launches)
        return fail(ADMM_E_INVALID, "bad profile query");
    std::lock_guard<std::mutex> lk(g_prof.mu);
    *total_ms = g_prof.ms[kernel_class];
    *launches = g_prof.n[kernel_class];
    return ADMM_OK;
}

int admm_clamp_backward_f32(const float* x, const float* dy, float* dx, size_t n, float lo, float hi, void* stream) {
    if (n == 0) return ADMM_OK;
    if (!x || !dy || !dx) return fail(ADMM_E_INVALID, "admm_clamp_backward_f32: NULL pointer");
    const size_t blocks = (n + 4 * 256 - 1) / (4 * 256);
    hipLaunchKernelGGL(admm::clamp_bwd_kernel, dim3((unsigned)(blocks < 65535 * 8 ? blocks : 65535 * 8)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, dy, dx, n, lo, hi);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ADMM_E_HIP, "admm_clamp_backward_f32: %s", hipGetErrorString(e));
    return ADMM_OK;
}

int admm_copy_async(void* dst, const void* src, size_t bytes, void* stream) {
    if (bytes == 0) return ADMM_OK;
    if (!dst || !src) return fail(ADMM_E_INVALID, "admm_copy_async: NULL pointer");
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(ADMM_E_HIP, "admm_copy_async: %s", hipGetErrorString(e));
    return ADMM_OK;
}

static_assert(sizeof(hipIpcMemHandle_t) == ADMM_IPC_HANDLE_BYTES, "hipIpcMemHandle_t size");

int admm_ipc_get_handle(const void* dev_ptr, void* handle_out, size_t* offset_out) {
    if (!dev_ptr || !handle_out || !offset_out) return fail(ADMM_E_INVALID, "admm_ipc_get_handle: NULL pointer");
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    hipError_t e = hipMemGetAddressRange(&base, &size, const_cast<void*>(dev_ptr));
    if (e != hipSuccess) return fail(ADMM_E_HIP, "admm_ipc_get_handle: hipMemGetAddressRange: %s", hipGetErrorString(e));
    hipIpcMemHandle_t h;
    e = hipIpcGetMemHandle(&h, base);
    if (e != hipSuccess) return fail(ADMM_E_HIP, "admm_ipc_get_handle: hipIpcGetMemHandle: %s", hipGetErrorString(e));
    std::memcpy(handle_out, &h, sizeof(h));
    *offset_out = static_cast<size_t>(static_cast<const char*>(dev_ptr) - static_cast<const char*>(base));
    return ADMM_OK;
}

int admm_ipc_open(const void* handle, int device, void** dev_ptr_out) {
    if (!handle || !dev_ptr_out) return fail(ADMM_E_INVALID, "admm_ipc_open: NULL pointer");
    int prev = -1;
    hipError_t e = hipGetDevice(&prev);
    if (e == hipSuccess && prev != device) e = hipSetDevice(device);
    if (e != hipSuccess) return fail(ADMM_E_HIP, "admm_ipc_open: select device %d: %s", device, hipGetErrorString(e));
    hipIpcMemHandle_t h;
    std::memcpy(&h, handle, sizeof(h));
    void* p = nullptr;
    e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
    if (prev != device) (void)hipSetDevice(prev);
    if (e != hipSuccess) return fail(ADMM_E_HIP, "admm_ipc_open: hipIpcOpenMemHandle on device %d: %s", device, hipGetErrorString(e));
    *dev_ptr_out = p;
    return ADMM_OK;
}

int admm_ipc_close(void* dev_ptr, int device) {
    if (!dev_ptr) return fail(ADMM_E_INVALID, "admm_ipc_close: NULL pointer");
    int prev = -1;
    hipError_t e = hipGetDevice(&prev);
    if (e == hipSuccess && prev != device) e = hipSetDevice(device);
    if (e != hipSuccess) return fail(ADMM_E_HIP, "admm_ipc_close: select device %d: %s", device, hipGetErrorString(e));
    e = hipIpcCloseMemHandle(dev_ptr);
    if (prev != device) (void)hipSetDevice(prev);
    if (e != hipSuccess) return fail(ADMM_E_HIP, "admm_ipc_close: %s", hipGetErrorString(e));
    return ADMM_OK;
}

int admm_tvd_grouped_workspace_bytes(int M, int N, int P, int B, int gb, int gp, int kh, int kw, int iso,
                                     size_t* out_bytes) {
    if (!out_bytes) return fail(ADMM_E_INVALID, "out_bytes is NULL");
    const int rc = check_grouped(M, N, P, B, gb, gp, kh, kw, iso);
    if (rc) return rc;
    *out_bytes = make_grouped_layout(M, N, (size_t)P * B, gb * gp, kh > 0, iso_batch(iso)).total;
    return ADMM_OK;
}

// The grouped entry points: one Call with the grouping, validated by check_call.
#define ADMM_GROUPED(x)                                                                                             \
    Call{y, x, M, N, P, B, h, kh, kw, dev_sc(lambda, rho), iso, maxit, workspace, workspace_bytes, stream, nullptr, \
         gb, gp, nparam, kGrouped}

int admm_tvd_forward_grouped_dev_f32(const float* y, float* x_out, int M, int N, int P, int B, int gb, int gp,
                                     const float* h, int kh, int kw, const float* lambda, const float* rho, int nparam,
                                     int iso, int maxit, void* workspace, size_t workspace_bytes, void* stream) {
    return forward_grouped(ADMM_GROUPED(x_out));
}

int admm_tvd_grouped_backward_workspace_bytes(int M, int N, int P, int B, int gb, int gp, int kh, int kw, int iso,
                                              int maxit, int rec_flags, size_t* out_bytes) {
    if (!out_bytes) return fail(ADMM_E_INVALID, "out_bytes is NULL");
    const int rc = check_grouped(M, N, P, B, gb, gp, kh, kw, iso);
    if (rc) return rc;
    if (no_plane_mode(iso, "the grouped adjoint")) return ADMM_E_UNSUPPORTED;
    if (maxit < 0) return fail(ADMM_E_INVALID, "maxit must be >= 0");
    // the larger of a pair per group (the larger (rho_bar, tau_bar) partial block) and one pair (more rows per part)
    Call c = shape_call(M, N, P, B, kh, kw, iso, maxit);
    c.kind = kGrouped, c.gb = gb, c.gp = gp;
    const PathPlan pl = plan_paths(adjoint_in(c, 1, rec_flags, Grads{}));
    c.nparam = gb * gp;
    const size_t a = adjoint_layout(c, pl).total;
    c.nparam = 1;
    const size_t b = adjoint_layout(c, pl).total;
    *out_bytes = a > b ? a : b;
    return ADMM_OK;
}

int admm_tvd_forward_grouped_record_dev_f32(const float* y, float* x_out, int M, int N, int P, int B, int gb, int gp,
                                            const float* h, int kh, int kw, const float* lambda, const float* rho,
                                            int nparam, int iso, int maxit, int rec_flags, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    return run_backward(1, rec_flags, ADMM_GROUPED(x_out), Grads{});
}

int admm_tvd_backward_grouped_recorded_dev_f32(const float* y, const float* x_bar, float* y_bar, float* h_bar,
                                               float* lambda_bar, float* rho_bar, int M, int N, int P, int B, int gb,
                                               int gp, const float* h, int kh, int kw, const float* lambda,
                                               const float* rho, int nparam, int iso, int maxit, const float* x_out,
                                               void* workspace, size_t workspace_bytes, void* stream) {
    return run_backward(2, 0, ADMM_GROUPED(const_cast<float*>(x_out)), Grads{x_bar, y_bar, h_bar, lambda_bar, rho_bar});
}

int admm_tvd_backward_grouped_dev_f32(const float* y, const float* x_bar, float* y_bar, float* h_bar, float* lambda_bar,
                                      float* rho_bar, int M, int N, int P, int B, int gb, int gp, const float* h, int kh,
                                      int kw, const float* lambda, const float* rho, int nparam, int iso, int maxit,
                                      float* x_out, void* workspace, size_t workspace_bytes, void* stream) {
    return run_backward(3, 0, ADMM_GROUPED(x_out), Grads{x_bar, y_bar, h_bar, lambda_bar, rho_bar});
}
#undef ADMM_GROUPED

int admm_tvd_state_workspace_bytes(int M, int N, int P, int B, int kh, int kw, int iso, size_t* out_bytes) {
    if (!out_bytes) return fail(ADMM_E_INVALID, "out_bytes is NULL");
    const int rc = check_state_shape(M, N, P, B, kh, kw, iso);
    if (rc) return rc;
    if (no_plane_mode(iso, "the state call")) return ADMM_E_UNSUPPORTED;
    // (the plain forward of the same arguments fits too: its MALL chunk schedule never needs more than the whole batch)
    *out_bytes = std::max(make_state_layout(M, N, (size_t)P * B, kh > 0, iso != 0).total,
                          forward_setup(shape_call(M, N, P, B, kh, kw, iso)).bytes);
    return ADMM_OK;
}

int admm_tvd_forward_state_dev_f32(const float* y, float* x_out, int M, int N, int P, int B, const float* h, int kh,
                                   int kw, const float* lambda, const float* rho, int iso, int maxit,
                                   const float* state_in, float* state_out, float* resid_out, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    const int rc = check_dev_scalars(lambda, rho);
    if (rc) return rc;
    return forward_state(Call{y, x_out, M, N, P, B, h, kh, kw, dev_sc(lambda, rho), iso, maxit, workspace, workspace_bytes,
                              stream, nullptr, 1, 1, 1, kState},
                         state_in, state_out, resid_out);
}

int admm_tvd_multi_workspace_bytes(int M, int N, int P, int B, int nbranch, int maxit, int flags, size_t* out_bytes) {
    if (!out_bytes) return fail(ADMM_E_INVALID, "out_bytes is NULL");
    int rc = check_multi(M, N, P, B, nbranch, maxit, flags);
    if (rc) return rc;
    *out_bytes = make_multi_layout(multi_call(M, N, P, B, nbranch, maxit, flags)).total;
    return ADMM_OK;
}

int admm_tvd_forward_multi_dev_f32(const float* y, float* x_out, int M, int N, int P, int B, int nbranch,
                                   const float* const* lambda, const float* const* rho, int maxit, int flags,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    Call c = multi_call(M, N, P, B, nbranch, maxit, flags);
    c.y = y, c.x_out = x_out, c.lam_b = lambda, c.rho_b = rho;
    c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.stream = stream;
    return forward_multi(c);
}

int admm_tvd_backward_multi_recorded_dev_f32(const float* x_bar, float* y_bar, float* lambda_bar, float* rho_bar, int M,
                                             int N, int P, int B, int nbranch, int maxit, const float* x_out,
                                             void* workspace, size_t workspace_bytes, void* stream) {
    Call c = multi_call(M, N, P, B, nbranch, maxit, 0);
    c.x_out = const_cast<float*>(x_out);   // (a replay reads x_out, the recorded forward's output)
    c.workspace = workspace, c.workspace_bytes = workspace_bytes, c.stream = stream;
    return backward_multi(c, Grads{x_bar, y_bar, nullptr, lambda_bar, rho_bar});
}

}  // extern "C"
