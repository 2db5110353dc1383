// capi_internal.hpp -- declarations shared by the library's host translation units:
//   admm_capi.hip   the extern "C" ABI (include/admm_deconv.h): argument validation, workspace layouts and
//                   queries, the recordings registry, the profiler API, the output transport (copy / IPC)
//   admm_paths.hip  the path decision table (plan_paths) with the one mapping from a Call to its input, the path
//                   queries, the library options and the tile-size policy
//   admm_launch.hip launch sequencing of the 2-pass / runtime-length / CU-resident / fused paths (the only TU
//                   that includes the 2-pass kernels): one 2-pass forward and one reverse sweep for every caller,
//                   one adjoint driver for single and grouped calls
// A call of any family (single, grouped, state, multi-branch) crosses these layers as one Call (and one Grads) by
// const reference.
// Reference interface: tvd_fft / tvd_fft_gpu, /root/reference/src/ops/ops.jl:99-188.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/admm_deconv.h"
#include "layout.hpp"
#include "plane_api.hpp"
#include "scalar_src.hpp"

namespace admm_capi {

using namespace admm::layout;
constexpr int kGenMax = 4096;

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// ---- options and tile policy (admm_paths.hip) ----
int opt(int k);
bool fused_enabled();
bool fused_adj_enabled();
int line_T(int M, int N);
size_t line_lds(int M, int T);
size_t fwdinv_lds(int M, int T);
int column_threads(int N);
int column_KB(int M, int N);
int bwd_line_T(int M, int N, bool iso);
size_t column_lds(int N, int KB);
size_t iso_a_lds(int M, int T);
size_t iso_b_lds(int M, int T);
int gen_T(int M, int N);
int gen_nb(int N, int T);
int gen_KB(int M, int N);
size_t gen_lds_line(int M, int T, bool upd);
size_t gen_lds_col(int N, int KB);

// ---- profiler (admm_capi.hip owns g_prof) ----
struct Prof {
    bool on = false;
    double ms[ADMM_K_COUNT] = {};
    long long n[ADMM_K_COUNT] = {};
    std::mutex mu;
};
extern Prof g_prof;

struct PendingEv {
    int cls;
    hipEvent_t a, b;
};

struct Launcher {
    hipStream_t s;
    bool prof;
    std::vector<PendingEv> ev;
    // `launch` may return void or an int status: the template dispatchers (launch_line, launch_column,
    // ...) return non-zero when no instance matches the requested tile, in which case nothing was
    // enqueued and the call must fail instead of returning unwritten outputs.
    template <typename F>
    int run(int cls, F&& launch) {
        PendingEv p{cls, nullptr, nullptr};
        if (prof) {
            hipEventCreate(&p.a);
            hipEventCreate(&p.b);
            hipEventRecord(p.a, s);
        }
        int lrc = 0;
        hipError_t e = hipSuccess;
        using R = decltype(launch());
        if constexpr (std::is_void_v<R>) {
            launch();
        } else if constexpr (std::is_same_v<R, hipError_t>) {
            e = launch();   // the plane launchers report hipGetLastError() themselves
        } else {
            lrc = (int)launch();
        }
        if (e == hipSuccess) e = hipGetLastError();
        if (prof) {
            hipEventRecord(p.b, s);
            ev.push_back(p);
        }
        if (e != hipSuccess) return fail(ADMM_E_HIP, "kernel launch (class %d) failed: %s", cls, hipGetErrorString(e));
        if (lrc != 0) return fail(ADMM_E_UNSUPPORTED, "no kernel instance for this tile (class %d, status %d)", cls, lrc);
        return ADMM_OK;
    }
    int finish() {
        if (!prof) return ADMM_OK;
        hipError_t e = hipStreamSynchronize(s);
        std::lock_guard<std::mutex> lk(g_prof.mu);
        for (auto& p : ev) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
                g_prof.ms[p.cls] += ms;
                g_prof.n[p.cls] += 1;
            }
            hipEventDestroy(p.a);
            hipEventDestroy(p.b);
        }
        ev.clear();
        if (e != hipSuccess) return fail(ADMM_E_HIP, "stream sync failed: %s", hipGetErrorString(e));
        return ADMM_OK;
    }
};

int check_shape(int M, int N, int P, int B, int kh, int kw, int iso);

// The prox of a call from its `iso` argument (ADMM_ISO_*): any non-zero value but ADMM_ISO_PLANE is the reference's
// batch-coupled BT.  ADMM_ISO_PLANE (BT of each pixel's own 2-vector, admm_plane_bt.hip) couples nothing: layouts,
// chunking and sequences are the anisotropic ones (every `bool iso` below is iso_batch), with the block-threshold
// line kernels in place of the ST ones; it runs the 2-pass / runtime-length kernels only (plan_paths).
inline bool iso_batch(int iso) { return iso != 0 && iso != ADMM_ISO_PLANE; }
inline bool iso_plane(int iso) { return iso == ADMM_ISO_PLANE; }
// entry points without a per-plane isotropic form
int no_plane_mode(int iso, const char* who);

// Planes per launch sequence.  The 2-pass kernels index planes by blockIdx.y (<= 65535), so a larger
// anisotropic forward runs as consecutive chunks of this many planes through one chunk-sized workspace
// (planes are independent, ops.jl:168-173).  A multiple of 256: every chunk but the last fills whole
// waves of the fused kernel (one workgroup per CU).
constexpr size_t kChunkPlanes = 255 * 256;
inline size_t launch_planes(size_t planes) { return planes < kChunkPlanes ? planes : kChunkPlanes; }
// The isotropic prox couples the whole batch through the per-pixel norm (ops.jl:6), so an isotropic
// batch is never split: it runs as one launch sequence of up to 65535 planes (check_shape's limit).
inline size_t chunk_planes(size_t planes, bool iso) { return iso ? planes : launch_planes(planes); }

// MALL-resident schedule of the anisotropic 2-pass forward (ADMM_OPT_MALL_STREAMS, DESIGN.md s5 "Round 6, c4"):
// planes in chunks of `chunk`, `streams` chunks in flight (the caller's stream + library streams), each chunk's
// per-iteration working set kept in the 256 MiB Infinity Cache.  streams = 1: the plain chunking above.
struct ChunkPlan {
    size_t chunk;
    int streams;
};
// the library's own streams on the current device (created once; non-blocking)
hipStream_t lib_stream(int i);

// Trajectory recorded by the forward for the backward (all optional).
struct Traj {
    float* s = nullptr;      // (K-1) x planes x 2 x M x N : s_k for k = 1..K-1
    float2* v = nullptr;     // K x planes x N x M/2        : forward dim-2 spectra (h_bar only)
    double2* sig = nullptr;  // (M/2+1) x N                 : top-left PSF spectrum (h_bar only)
    float* nrm = nullptr;    // (K-1) x M x N               : isotropic batch norm of s_k (iso only)
    unsigned* m = nullptr;   // (K-1) x planes x 16 x 512   : ST mask bytes of s_k instead of s (fused only)
    bool iso_lane = false;   // isotropic 256 x 256: s and nrm lane-native (plane_iso.hip), for the fused adjoint
};

// ---- path selection (admm_paths.hip): ONE decision table for every entry point -----------------------------------------------
// Which kernels a call runs is decided in plan_paths and nowhere else, for every family; admm_launch.hip only executes
// the plan, and the admm_query_* entries return it to tests without a GPU.
// Inputs: shape, prox, PSF, what the call is (plain forward, recording with ADMM_REC_* flags, combined backward with or
// without h_bar / rho_bar), its family and the library options.  A family does not choose kernels: it states what it
// asks of them (PathIn::needs), and every rule of the table states what its kernels can take.
enum CallKind { kSingle, kGrouped, kState, kMulti };
enum PathCap : unsigned {
    kCapGroups = 1,     // a plane -> group map (a PSF, lambda and rho per group)
    kCapState = 2,      // a caller-given s_0
    kCapPlaneBT = 4,    // ADMM_ISO_PLANE: the block-threshold line kernels
    kCapBranches = 8,   // several branches in one grid
};
struct PathIn {
    int M, N;
    bool iso, psf;
    int mode;            // ADMM_MODE_FORWARD, ADMM_MODE_RECORD, ADMM_MODE_BACKWARD
    int rec_flags;       // ADMM_REC_* (record)
    bool h_bar, rho_bar; // backward: gradients asked for
    size_t planes;       // planes of the call's grid (0: unknown or sharded, no plane-count rule)
    bool bt;             // ADMM_ISO_PLANE (iso is then false)
    CallKind kind;
    unsigned needs() const {
        return (kind == kGrouped ? kCapGroups : kind == kState ? kCapState : kind == kMulti ? kCapBranches : 0u) |
               (bt ? kCapPlaneBT : 0u);
    }
};
enum MinPlanesFor { kMinFused, kMinFusedIso, kMinResident, kMinResidentIso };
struct PathPlan {
    bool want_h = false;     // the forward records the dim-2 spectra h_bar needs (2-pass column pass)
    bool ln_traj = false;    // the fused 256^2 forward records s lane-native
    bool masks = false;      // ADMM_REC_MASKS honoured: ST mask bits (aniso) / lane-native s and |s| (iso)
    bool iso_lane = false;   // the fused isotropic trajectory + sweep
    int fwd = 0;             // ADMM_PATH_* of the forward
    int bwd = 0;             // ADMM_PATH_SWEEP_* of the reverse sweep (0: none)
};
// the trajectory a recording keeps, as run_forward sees it (pointers only matter as null / non-null)
struct TrajFlags {
    bool s, v, nrm, m, iso_lane;
};
PathPlan plan_paths(const PathIn& q);

// ---- backward workspace (admm_capi.hip) ----
// backward workspace = forward layout + trajectory + reverse-sweep buffers
struct BwdLayout {
    Layout f;
    size_t traj_s, traj_v, sig, sbA, sbB, vsum, rpart, Qp, Q, hpart, hcorr, hA, rt, total;
    size_t traj_n, wbar, Rmap, Rpart;   // isotropic only
    size_t rtmp;                        // two-stage column sums (kRedParts x columns doubles)
    int nblk_line, nblk_corr, TY;
    int nblk_isoA, nblk_isoR;           // isotropic: per-step partial rows = nblk_isoA + nblk_isoR
    // a grouped call (make_grouped_bwd_layout), zero otherwise: the split partials of the group-segmented sums and the
    // parts a group's (rho_bar, tau_bar) rows / h_bar correlation rows are summed in
    size_t gtmp;
    int split_rt, split_h;
};

constexpr int kIsoAdjRBlocks = 256;     // ISO_ADJ_R grid (tau_bar partial rows per step)
constexpr int kRedParts = 256;          // first-stage blocks per column of a long column sum

BwdLayout make_bwd_layout(int M, int N, size_t planes, int kh, int kw, int maxit, bool want_h, bool iso,
                          bool masks = false);

// ---- several branches in one grid (admm_capi.hip) ----
// Workspace: per branch {tau, rho, lambda} (16 B each, one block), its C table and its lane-native tables;
// per grid plane the fused kernel's H^T y (= y) and s state, the trajectory (full s_k or mask bytes), the
// reverse sweep's sbar and Vsum state and the (rho_bar, tau_bar) partials.  After the forward, the H^T y
// slots hold each branch's Vsum (natural layout, y_bar only) and the s slots D x_K (rho_bar only).
struct MultiLayout {
    size_t prm, twM, twN, C, F, hln, sln, traj, sbar, vsl, part, rt, rtmp, total;
    size_t fmap, qpart, nrm, rmap;   // isotropic (ADMM_MULTI_ISO): f maps, q / R partials, |s| slots, R maps
    // Below the plane-count rule the branches run the 2-pass kernels in one grid (two_pass, from the plan): spectra, s
    // state (anisotropic: sA / sbA ping-pong), and for the reverse sweep sbar (two), Vsum and (isotropic) vbar and
    // the plane-group R partials; qpart then holds the plane-group |s|^2 partials, traj / nrm the natural-layout
    // s_k / |s_k| slots (|s_k| per branch), part the (rho_bar, tau_bar) rows of every branch (pbs doubles apart,
    // rows_b per step)
    bool two_pass;
    size_t spec0, spec1, sA, sbA, sbB, vsum, wbar, Rpart, pbs;
    int ngb, G, rows_b, nblk_a;
};
constexpr int kMultiM = 256, kMultiN = 256;
size_t multi_C_bytes();
size_t multi_F_bytes();
size_t multi_iso_rows(int K);

// ---- resumable solve (admm_tvd_forward_state_dev_f32) ----
// What a state call reads and writes besides y and x_out (null: not given / not wanted), and its own workspace slots
// behind the forward layout: the start kernel's v_0 plane set, the batch factor map of s_K (isotropic residuals) and
// the residual pass's block sums.
struct StateIO {
    const float* in;   // s_0, natural layout (planes x 2 x N x M)
    float* out;        // s_K
    float* resid;      // planes x 4
    float* v0;
    float* fmapK;
    double* rpart;
    float* sK;         // the fused path's s_K when state_out is not wanted (residuals only), natural layout
};

// ---- the call descriptor ----
// What a solve is.  Every extern "C" entry point fills one in once (the shape-only workspace and path queries with the
// fields they have), and everything below the ABI receives it by const reference.
struct Call {
    const float* y;
    float* x_out;
    int M, N, P, B;
    const float* h;           // a grouped call: one PSF per group, consecutive
    int kh, kw;
    admm::ScalarSrc sc;       // a grouped call: lam / rho point at nparam device values
    int iso, maxit;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
    const admm_batch_reducer* red;   // the batch reducer, only where it acts: isotropic and fn set
    int gb = 1, gp = 1, nparam = 1;  // the grouping (admm_tvd_*_grouped_*); a single solve: one group, one pair
    CallKind kind = kSingle;         // the family: what the call asks of its kernels (PathIn::needs)
    const StateIO* st = nullptr;     // a state call: never the smooth-length kernels, warm start when st->in is set
    // a multi-branch call (admm_tvd_*_multi_*): nbranch solves of the same P x B planes in one grid, branch i with the
    // device scalars lam_b[i] / rho_b[i] (host arrays; sc is not used), its ADMM_MULTI_* / ADMM_REC_* flags
    int nbranch = 1;
    const float* const* lam_b = nullptr;
    const float* const* rho_b = nullptr;
    int flags = 0;
    bool grouped() const { return kind == kGrouped; }
    size_t planes() const { return (size_t)P * B; }              // input planes
    size_t grid_planes() const { return planes() * nbranch; }    // planes solved: every branch's
    int groups() const { return gb * gp; }
};
// What an adjoint reads (x_bar) and writes (null: not wanted); all null for a recording forward.  lambda_bar / rho_bar:
// one value per (lambda, rho) pair of the call -- nparam of a grouped call, nbranch of a multi-branch one.
struct Grads {
    const float* x_bar;
    float *y_bar, *h_bar, *lambda_bar, *rho_bar;
};

// ---- from a call to its plan (admm_paths.hip) ----
// The one mapping from a Call to the decision table's input, per direction; every solve, workspace size and path query
// goes through it, so the three take the same plan.  forward_in: a plain forward (a multi-branch call: its forward with
// or without ADMM_MULTI_RECORD).  adjoint_in: phases as run_backward's (1 recording, 2 replay, 3 combined), rec_flags
// the recording's request, g the gradients asked for, rec_masks the masks flag of the recording a replay found.
Call shape_call(int M, int N, int P, int B, int kh, int kw, int iso, int maxit = 0);   // a shape-only entry's Call
PathIn forward_in(const Call& c);
PathIn adjoint_in(const Call& c, int phases, int rec_flags, const Grads& g, bool rec_masks = false);
// the chunk schedule of a forward of `planes` planes planned as pl (q.planes is 0 for a sharded call)
ChunkPlan forward_chunks(const PathIn& q, const PathPlan& pl, size_t planes);

// ---- workspace carving ----
struct Carver {
    size_t off;
    size_t take(size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes);
        return o;
    }
};

// ---- grouped solve (admm_tvd_forward_grouped_dev_f32) ----
// Planned by plan_paths on the rules whose kernels take the plane -> group map (kCapGroups); one launch sequence over
// the whole batch, never the MALL chunk schedule.
// floats (C) / float2 (G) between the groups' 2-pass tables
inline unsigned group_tab_f(int M, int N) { return (unsigned)(align_up((size_t)(M / 2 + 1) * N * 4) / 4); }
// Workspace: the single-PSF forward layout of the whole batch, and behind it G consecutive blocks of each table
// (group_tab_f floats of C, as many float2 of G and grouped_tables_bytes() of lane-native tables per group; one 16-byte
// scalar block per group).  The layout's own scalar / C / G / lane-native slots stay allocated and are not used (one
// table set, about 0.8 MB at 256 x 256); prm, C, G and F name group 0's appended blocks instead.
Layout make_grouped_layout(int M, int N, size_t planes, int groups, bool psf, bool iso);

// ---- grouped adjoint (admm_tvd_backward_grouped_*) ----
// Planned by plan_paths too (reported by admm_query_grouped_paths): no fused reverse sweep takes the group map, so masks
// and iso_lane stay false and a fused forward's lane-native trajectory (ln_traj) is swept by sweep_2pass.
// Workspace: a BwdLayout of the whole batch, behind it the grouped table blocks of make_grouped_layout and, per group,
// sig (PSF spectrum), Q, hcorr, hA and rt; f.prm / C / G / F and sig / Q / hcorr / hA / rt name those blocks (the
// layout's own single-set slots stay allocated and unused).  gtmp: the split partials of the group-segmented sums.
BwdLayout make_grouped_bwd_layout(const Call& c, bool want_h);
// parts for a fixed-order sum of n rows: about 4096 rows per block, at most 256 parts
inline int group_split(long long n) {
    const long long p = (n + 4095) / 4096;
    return p < 1 ? 1 : p > 256 ? 256 : (int)p;
}

// ---- resumable solve: workspace ----
// Planned by plan_paths on the rules whose kernels can start from a given s_0 (kCapState; reported by
// admm_query_state_path); one launch sequence over the whole batch.
// Workspace: the forward layout of the whole batch, then v_0, the factor map of s_K (isotropic), the residual block
// sums and (256 x 256 anisotropic) a natural-layout s_K for a fused call that wants residuals without state_out.
struct StateLayout {
    Layout f;
    size_t v0, fmapK, rpart, sK, total;
};
StateLayout make_state_layout(int M, int N, size_t planes, bool psf, bool iso);

// ---- launch sequencing (admm_launch.hip) ----
// The entry points below set a call up and run the path it was planned on; the 2-pass kernels' step sequences exist
// once (two_pass_forward / two_pass_reverse on a TwoPass grid: a single or grouped solve, or the one-grid call's
// branches), as do the isotropic norm step, the fused isotropic loops and the gradient assembly.
// run_forward: np planes of the call from plane p0 on (default: all of them), through the layout `lay` at `ws`.  A
// grouped call (c.grouped()): h holds one PSF per group, sc.lam / sc.rho point at nparam device values, lay is
// make_grouped_layout's (or a grouped BwdLayout's f); the setup kernels run over the groups.
// tables = false: the workspace already holds this call's twiddles, C / G tables and scalar block (a later plane
// chunk of the same call through the same chunk workspace): the setup kernels are not launched again
int run_forward(Launcher& ln, const Call& c, unsigned char* ws, const Layout& lay, const Traj& tr, int fwd_path,
                bool tables = true, size_t p0 = 0, size_t np = 0);
// everything run_backward does after validating the call and updating the recordings registry: phases & 1 the
// recording forward, phases & 2 the reverse sweep and the assembly of the gradients; a single or a grouped call
int launch_backward(int phases, const Call& c, const Grads& g, const PathPlan& plan, const BwdLayout& bl);
// a state call (c.st set): the forward on `path` from s_0 or the zero state, then the end kernels (s_K, residual norms)
int launch_forward_state(const Call& c, const StateLayout& L, int path);
// a multi-branch call on the grid its layout was planned for (L.two_pass): the forward (recording with
// ADMM_MULTI_RECORD in c.flags), and the reverse sweep of such a recording (c.x_out: the recorded forward's output)
int launch_forward_multi(const Call& c, const MultiLayout& L);
int launch_backward_multi(const Call& c, const Grads& g, const MultiLayout& L);

}  // namespace admm_capi
