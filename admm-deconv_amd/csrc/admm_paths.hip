// admm_paths.hip -- the path decision table and the library options (host code only; see capi_internal.hpp).
// Which kernels a call runs -- single, grouped, state or multi-branch, either isotropic mode -- is decided in plan_paths
// and nowhere else: two rule lists (reverse sweep, forward), each rule with the capabilities of its kernels.
// forward_in / adjoint_in are the one way from a Call to the table's input; admm_launch.hip executes the plan and the
// admm_query_* entries return it to tests without a GPU.  The tile-size policy of the 2-pass and runtime-length
// kernels lives here too: the workspace layouts (admm_capi.hip) and the launches (admm_launch.hip) share it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "capi_internal.hpp"
#include "fft_reg.hpp"
#include "resident_api.hpp"
#include "smooth_api.hpp"

namespace admm_capi {

// Library options (admm_set_option; process-global, read at each call).  The defaults are the tuned
// choices; the others exist for tests (fused vs 2-pass) and tuning experiments.  A recording stores
// the option values it was made with, and its replay rejects a change (RecTag below).
std::atomic<int> g_opt[ADMM_OPT_COUNT] = {{1}, {1}, {0}, {0}, {0}, {0}, {0}, {1}, {1}, {-1}, {4}};
int opt(int k) { return g_opt[k].load(std::memory_order_relaxed); }

// ADMM_OPT_FUSED = 0 forces the 2-pass path (tests compare the two).
bool fused_enabled() { return opt(ADMM_OPT_FUSED) != 0; }
// ADMM_OPT_FUSED_ADJ = 0 keeps the 2-pass reverse sweep (line_adj + column) on a fused trajectory
bool fused_adj_enabled() { return opt(ADMM_OPT_FUSED_ADJ) != 0; }

// ---- tile-size policy ------------------------------------------------------------------------
// T = lines per line-kernel block (power of two dividing N); KB = slots per column-kernel block.
int line_T(int M, int N) {
    int pref = M <= 512 ? 8 : 4;
    const int v = opt(ADMM_OPT_LINE_T);
    if (v == 2 || v == 4 || v == 8 || v == 16) pref = v < pref ? v : pref;
    return N < pref ? N : pref;
}
size_t line_lds(int M, int T) {
    const size_t L = M / 2;
    return (size_t)M * 8 + 3 * (size_t)(T + 2) * L * 8;
}
size_t fwdinv_lds(int M, int T) { return (size_t)M * 8 + 2 * (size_t)T * (M / 2) * 8; }
int max_q(int NN) {
    switch (NN) {
#define X(v) case v: return admm::plan_max_q<v, false>();
        X(2) X(4) X(8) X(16) X(32) X(64) X(128) X(256) X(512) X(1024)
#undef X
    }
    return NN;
}
// column block size: 1024 threads for long columns, so that a block covers >= 64 B of every row
// (256 threads at N = 512 gave 4 slots = 32 B per row); ADMM_OPT_COL_THREADS overrides (256 or 1024)
int column_threads(int N) {
    int nt = N >= 512 ? 1024 : 256;
    const int v = opt(ADMM_OPT_COL_THREADS);
    if (v == 256 || ((v == 512 || v == 1024) && N >= 256)) nt = v;
    return nt;
}
int column_KB(int M, int N) {
    int KB = column_threads(N) / max_q(N);
    if (KB > M / 2) KB = M / 2;
    if (KB > 32) KB = 32;
    return KB;
}
// reverse sweep line tile: the isotropic adjoint kernels (ISO_ADJ_A / _B) run best with 4 lines per
// block (c5 iso: 55.4 -> 51.9 ms of adjoint per step, tools/iso_knobs.sh); the rest keeps line_T
int bwd_line_T(int M, int N, bool iso) {
    const int t = line_T(M, N);
    return iso && t > 4 ? 4 : t;
}
size_t column_lds(int N, int KB) { return (size_t)N * 16 + (size_t)KB * (N + 1) * 8; }
size_t iso_a_lds(int M, int T) { return (size_t)M * 8 + 3 * (size_t)(T + 1) * (M / 2) * 8; }
size_t iso_b_lds(int M, int T) { return (size_t)M * 8 + (size_t)(2 * T + 1) * M * 4 + 2 * (size_t)T * (M / 2) * 8; }

// Plane counts from which the one-workgroup-per-plane paths beat the 2-pass kernels (ADMM_OPT_MIN_PLANES = -1).
// A per-plane grid uses one CU per plane for the whole solve, so below about one CU wave it leaves CUs idle
// while the 2-pass kernels spread every plane over many workgroups.  Measured on MI355X (tools/time_small.py,
// profiles/r04_small_batch_paths.jsonl; K = 25 forward, K = 50 recording + sweep):
//   fused 256^2 anisotropic  forward 96 planes 1.32 vs 1.34 ms, 64: 1.29 vs 1.07; recording + sweep 96: 5.55 vs
//                            6.24, 64: 5.34 vs 4.75  -> 96
//   fused_iso 256^2          128: 2.03 vs 2.13, 64: 1.84 vs 1.40  -> 112
//   resident 250^2           192: 2.53 vs 2.96, 128: 2.48 vs 1.99; 128^2 256: 0.88 vs 0.93, 128: 0.84 vs 0.62
//                            -> 192 for sides >= 128 (smaller sides: every batch, the per-plane latency is small)
//                            (sides < 128: 96^2 0.43 vs 0.40 at 1..16 planes, 64^2 and 32^2 faster at every count)
//   resident_iso             256 planes: 250^2 3.94 vs 5.78, 120^2 1.04 vs 1.53, 64^2 x 512 0.80 vs 0.96;
//                            250^2 x 64 4.41 vs 1.84 (before its A / B row walkers)  -> 256
bool enough_planes(const PathIn& q, MinPlanesFor which) {
    const int o = opt(ADMM_OPT_MIN_PLANES);
    if (q.planes == 0 || o == 0) return true;
    if (o > 0) return q.planes >= (size_t)o;
    switch (which) {
        case kMinFused: return q.planes >= 96;
        case kMinFusedIso: return q.planes >= 112;
        case kMinResident: return std::max(q.M, q.N) < 128 || q.planes >= 192;
        case kMinResidentIso: return q.planes >= 256;
    }
    return true;
}
// MALL-resident schedule (ADMM_OPT_MALL_STREAMS; DESIGN.md s5 "Round 6, c4").  A 2-pass iteration touches
// 28 B/px (packed spectrum in and out 8, s in and out 16, Y_h 4): at c4 (768 planes of 512^2) 5.6 GB per
// iteration, so every pass streams from HBM.  Chunks of ~224 MiB / n (8 planes at 512^2, n = 4) run all K
// iterations with n of them in flight: their sets stay in the 256 MiB Infinity Cache, and the n streams overlap
// each other's kernel tails.  tools/c4_chunk_probe.py, profiles/r06_c4_chunk_probe.jsonl: 81.8 -> 75.7 ms per c4
// solve (8 planes x 4 streams; 16 x 2 77.2, 8 x 2 97.8: one or two small grids alone leave the chip idle; 5-12
// streams 97-149 ms, profiles/r06_c4_mall_streams_sweep.txt -- their 4-5 plane chunks are too small: 4 x 4 97.0,
// 5 x 4 85.3 ms; with 8 hardware queues 6 / 8 streams are slower still, profiles/r06_c4_hw_queues_probe.txt).
// The smooth-length 2-pass kernels gain the same way (480 x 640 x 64 / 256 +5 / +7 %, 384^2 x 512 +11 %).
ChunkPlan forward_chunks(const PathIn& q, const PathPlan& pl, size_t planes) {
    const size_t base = chunk_planes(planes, q.iso);
    if (q.bt) return {base, 1};   // ADMM_ISO_PLANE: plain chunks, never the MALL schedule
    const int n = opt(ADMM_OPT_MALL_STREAMS);
    const bool two_pass = pl.fwd == ADMM_PATH_2PASS || pl.fwd == ADMM_PATH_SMOOTH || pl.fwd == ADMM_PATH_RUNTIME;
    if (q.iso || n <= 1 || !two_pass) return {base, 1};
    constexpr size_t kMall = size_t(256) << 20, kBudget = size_t(224) << 20;
    const size_t per_plane = 28 * (size_t)q.M * q.N;
    if (planes * per_plane <= 2 * kMall) return {base, 1};
    size_t chunk = kBudget / ((size_t)n * per_plane);
    // chunks of 1-2 large planes lose (2048^2 x 8: 1-plane chunks -15 %, 1000^2 x 64: 2-plane chunks -2 %;
    // profiles/r06_mall_generic_ab.jsonl): whole batch
    if (chunk < 4) return {base, 1};
    if (chunk > base) chunk = base;
    return {chunk, n > 16 ? 16 : n};
}

// ---- the decision table ------------------------------------------------------------------------------------------
// Two rule lists, the reverse sweep's and the forward's, first match wins.  A rule is a kernel family: `takes` is what
// its kernels can be handed (PathCap: a plane -> group map, a caller-given s_0, ADMM_ISO_PLANE, several branches in one
// grid), `applies` when they are the choice for a shape, a prox, the options and a plane count.  A call family
// (grouped, state, multi-branch; ADMM_ISO_PLANE) has no rules of its own: it is planned on the rules that take all it
// needs.  A new family is one more capability bit, set on the rules whose kernels were taught it.
struct Rule {
    int path;
    unsigned takes;
    bool (*applies)(const PathIn&, const TrajFlags&);
};
bool takes(const Rule& r, const PathIn& q) { return (q.needs() & ~r.takes) == 0; }
// the masks / lane-native isotropic trajectory: asked for by a recording (ADMM_REC_MASKS), taken by the combined call
// whenever rho_bar is not wanted
bool masks_asked(const PathIn& q) { return q.mode == ADMM_MODE_RECORD ? (q.rec_flags & ADMM_REC_MASKS) != 0 : !q.rho_bar; }

// The reverse sweep is chosen first: the trajectory it reads is what the forward must record (t.v: the dim-2 spectra of
// an h_bar recording, which only the 2-pass and runtime-length column passes keep).
const Rule kBwdRules[] = {
    // plane256_adj_kernel: the fused 256 x 256 forward's lane-native s_k, or their ST mask bits (one table set per
    // branch: no group map)
    {ADMM_PATH_SWEEP_FUSED, kCapBranches, [](const PathIn& q, const TrajFlags& t) {
         return fused_shape(q.M, q.N, q.iso) && !t.v && fused_enabled() && fused_adj_enabled() && enough_planes(q, kMinFused);
     }},
    // plane256_isoadj: the split-iteration trajectory (s and |s| lane-native); rho_bar cannot be formed from it, so only
    // where the masks flag allows
    {ADMM_PATH_SWEEP_FUSED_ISO, kCapBranches, [](const PathIn& q, const TrajFlags& t) {
         return q.iso && fused_tables_shape(q.M, q.N) && !t.v && fused_enabled() && fused_adj_enabled() &&
                enough_planes(q, kMinFusedIso) && masks_asked(q);
     }},
    {ADMM_PATH_SWEEP_RUNTIME_ISO, kCapGroups, [](const PathIn& q, const TrajFlags&) { return q.iso && generic_shape(q.M, q.N); }},
    {ADMM_PATH_SWEEP_RUNTIME, kCapGroups | kCapPlaneBT, [](const PathIn& q, const TrajFlags&) { return generic_shape(q.M, q.N); }},
    {ADMM_PATH_SWEEP_2PASS_ISO, kCapGroups | kCapBranches, [](const PathIn& q, const TrajFlags&) { return q.iso; }},
    // (also of a fused forward's lane-native trajectory: PathPlan::ln_traj)
    {ADMM_PATH_SWEEP_2PASS, kCapGroups | kCapPlaneBT | kCapBranches, [](const PathIn&, const TrajFlags&) { return true; }},
};

const Rule kFwdRules[] = {
    // runtime-length shapes: the CU-resident solve (admm_resident.hip) where compiled and measured faster,
    // anisotropic and recording neither dim-2 spectra, norms nor mask bits (it writes s_k into the slots)
    // (and the small power-of-two squares it compiled: 32, 64, 128; it needs no spectra buffers, so it runs on
    // either layout)
    {ADMM_PATH_RESIDENT, 0, [](const PathIn& q, const TrajFlags& t) {
         return !q.iso && !t.v && !t.nrm && !t.m && opt(ADMM_OPT_RESIDENT) != 0 &&
                (!generic_shape(q.M, q.N) || opt(ADMM_OPT_SMOOTH) != 0) &&
                admm::rs::has_shape(q.M, q.N, opt(ADMM_OPT_RESIDENT) >= 2) && enough_planes(q, kMinResident);
     }},
    // isotropic: the split-iteration CU-resident solve (resident_iso_kernel, one launch per iteration with the
    // norm kernel between); it records s_k and |s_k| in the natural layout the 2-pass / runtime sweeps read
    {ADMM_PATH_RESIDENT_ISO, 0, [](const PathIn& q, const TrajFlags& t) {
         return q.iso && !t.v && opt(ADMM_OPT_RESIDENT) != 0 && (!generic_shape(q.M, q.N) || opt(ADMM_OPT_SMOOTH) != 0) &&
                admm::rs::has_iso_shape(q.M, q.N, opt(ADMM_OPT_RESIDENT) >= 2) && enough_planes(q, kMinResidentIso);
     }},
    // compile-time-plan kernels when this build has either length (admm_smooth.hip), else runtime plans
    {ADMM_PATH_SMOOTH, 0, [](const PathIn& q, const TrajFlags&) {
         return generic_shape(q.M, q.N) && opt(ADMM_OPT_SMOOTH) != 0 &&
                (admm::sm::has_length(q.M) || admm::sm::has_length(q.N));
     }},
    {ADMM_PATH_RUNTIME, kCapGroups | kCapState | kCapPlaneBT,
     [](const PathIn& q, const TrajFlags&) { return generic_shape(q.M, q.N); }},
    // 256 x 256 anisotropic: one workgroup per plane runs all K iterations (plane_kernel.hip; its grouped recording and
    // state instances: plane_grouped_rec.hip, plane_state.hip)
    {ADMM_PATH_FUSED, kCapGroups | kCapState | kCapBranches, [](const PathIn& q, const TrajFlags& t) {
         return fused_shape(q.M, q.N, q.iso) && !t.v && fused_enabled() && enough_planes(q, kMinFused);
     }},
    // 256 x 256 isotropic: split-iteration per-plane kernels (plane_iso.hip); a recording only in its own
    // lane-native layout (the fused sweep's)
    {ADMM_PATH_FUSED_ISO, kCapBranches, [](const PathIn& q, const TrajFlags& t) {
         return q.iso && fused_tables_shape(q.M, q.N) && (!t.s || t.iso_lane) && !t.v && fused_enabled() &&
                enough_planes(q, kMinFusedIso);
     }},
    // the 2-pass kernels: every tuned shape and family, several 256 x 256 branches in one grid included (below the fused
    // kernels' plane counts over all branches: the c5 training step at batch 2 has 30, tools/small_batch_probe.py,
    // profiles/r05_small_batch_probe.jsonl)
    {ADMM_PATH_2PASS_ISO, kCapGroups | kCapState | kCapBranches, [](const PathIn& q, const TrajFlags&) { return q.iso; }},
    {ADMM_PATH_2PASS, kCapGroups | kCapState | kCapPlaneBT | kCapBranches,
     [](const PathIn&, const TrajFlags&) { return true; }},
};

template <size_t n>
int first_rule(const Rule (&rules)[n], const PathIn& q, const TrajFlags& t) {
    for (const Rule& r : rules)
        if (takes(r, q) && r.applies(q, t)) return r.path;
    return 0;
}

PathPlan plan_paths(const PathIn& q) {
    PathPlan pl;
    TrajFlags t{false, false, false, false, false};
    if (q.mode != ADMM_MODE_FORWARD) {
        pl.want_h = (q.mode == ADMM_MODE_RECORD ? (q.rec_flags & ADMM_REC_HBAR) != 0 : q.h_bar) && q.psf;
        t = TrajFlags{true, pl.want_h, q.iso, false, false};
        pl.bwd = first_rule(kBwdRules, q, t);
        // what the fused sweeps read instead of the natural-layout s_k: mask bits where asked for (anisotropic), the
        // split-iteration trajectory (isotropic)
        pl.iso_lane = pl.bwd == ADMM_PATH_SWEEP_FUSED_ISO;
        pl.masks = pl.iso_lane || (pl.bwd == ADMM_PATH_SWEEP_FUSED && masks_asked(q));
        t.m = pl.masks && !q.iso, t.iso_lane = pl.iso_lane;
    }
    pl.fwd = first_rule(kFwdRules, q, t);
    // the fused kernel records s in its lane-native layout, for the fused sweep or the 2-pass line adjoint
    pl.ln_traj = t.s && pl.fwd == ADMM_PATH_FUSED;
    return pl;
}

// ---- from a call to its plan ---------------------------------------------------------------------------------------
PathIn forward_in(const Call& c) {
    PathIn q{c.M, c.N, iso_batch(c.iso), c.kh > 0, ADMM_MODE_FORWARD, 0, false, false, c.grid_planes(), iso_plane(c.iso), c.kind};
    // a sharded isotropic solve plans without the plane-count rule: every shard must take the same path, since
    // the fused and 2-pass kernels hand the reducer their sum maps in different layouts (lane-native float2 vs
    // natural), and uneven shards can fall on either side of a threshold; so must its recording and its sweep
    if (c.red) q.planes = 0;
    // a multi-branch call records from its forward entry; no rho_bar from the ST mask bits, nor from the isotropic
    // recording (which is the masks trajectory).  Its reverse sweep runs on the grid of its forward (MultiLayout::
    // two_pass): only the forward of its plan is read.
    if (c.kind == kMulti && (c.flags & ADMM_MULTI_RECORD)) {
        q.mode = ADMM_MODE_RECORD;
        q.rec_flags = (c.flags & ADMM_REC_MASKS) || q.iso ? ADMM_REC_MASKS : 0;
    }
    return q;
}

Call shape_call(int M, int N, int P, int B, int kh, int kw, int iso, int maxit) {
    Call c{};
    c.M = M, c.N = N, c.P = P, c.B = B, c.kh = kh, c.kw = kw, c.iso = iso, c.maxit = maxit;
    return c;
}

PathIn adjoint_in(const Call& c, int phases, int rec_flags, const Grads& g, bool rec_masks) {
    PathIn q = forward_in(c);
    q.mode = phases == 3 ? ADMM_MODE_BACKWARD : ADMM_MODE_RECORD;
    // a replay (phase 2 alone) is planned as the recording it replays was: h_bar as the replay asks (its tag must match
    // the recording's), masks from the recording's tag
    q.rec_flags = phases != 2 ? rec_flags : (g.h_bar ? ADMM_REC_HBAR : 0) | (rec_masks ? ADMM_REC_MASKS : 0);
    q.h_bar = g.h_bar != nullptr, q.rho_bar = g.rho_bar != nullptr;
    return q;
}

// lines per block: the largest of 8, 4, 2, 1 dividing N with T * M <= 4096 (LDS ~ 24 T M bytes)
// options ADMM_OPT_GEN_TM (max T x M of a line block), ADMM_OPT_GEN_KN (max KB x N of a column block)
int gen_opt(int k, int dflt) {
    const int v = opt(k);
    return v >= 256 && v <= 8192 ? v : dflt;
}
int gen_T(int M, int N) {
    // 2048: smaller blocks, more of them resident per CU (480x640: 1.3x over 4096, tools/gen_knobs.sh).
    // T need not divide N (ragged last block): 250 x 250 ran 2-line blocks when it had to.
    const int tm = gen_opt(ADMM_OPT_GEN_TM, 2048);
    for (int t = 8; t > 1; t >>= 1)
        if (t * M <= tm && t <= N) return t;
    return 1;
}
// line blocks per plane: the last block of a plane may hold fewer than T lines (N need not divide by T)
int gen_nb(int N, int T) { return (N + T - 1) / T; }
int gen_KB(int M, int N) {
    // 1024 points per column block: with the XCD-aware block order, smaller blocks won at every size
    // measured (480x640 column pass 3.29 -> 2.92 ms; 256 / 512 / 2048+ slower, tools/time_generic.py)
    int kb = gen_opt(ADMM_OPT_GEN_KN, 1024) / N;
    kb = kb < 1 ? 1 : (kb > 16 ? 16 : kb);
    return kb > M / 2 + 1 ? M / 2 + 1 : kb;
}
// dynamic LDS of the runtime-length kernels: ping-pong FFT buffers (+ the two D^T channels of the
// update kernels) + the twiddle table staged by gen::stage_tw (8 n bytes, 8-B aligned)
size_t gen_lds_line(int M, int T, bool upd) {
    // A, B hold ceil(T / 2) paired complex transforms (gen::pack_real: two real lines per transform)
    const size_t base = (size_t)2 * ((T + 1) / 2) * M * 8 + (upd ? (size_t)(2 * T + 1) * M * 4 : 0);
    return ((base + 7) & ~size_t(7)) + (size_t)M * 8;
}
size_t gen_lds_col(int N, int KB) { return (size_t)2 * KB * N * 8 + (size_t)N * 8; }

}  // namespace admm_capi

using namespace admm_capi;

extern "C" {

int admm_set_option(int option, int value) {
    if (option < 0 || option >= ADMM_OPT_COUNT) return fail(ADMM_E_INVALID, "unknown option %d", option);
    g_opt[option].store(value, std::memory_order_relaxed);
    return ADMM_OK;
}

int admm_get_option(int option, int* value) {
    if (option < 0 || option >= ADMM_OPT_COUNT || !value) return fail(ADMM_E_INVALID, "bad option query %d", option);
    *value = opt(option);
    return ADMM_OK;
}

// The path queries: validate, map, plan, report.  A query has a shape, a prox, a PSF height and a plane count only.
static Call query_call(int M, int N, int iso, int kh, CallKind kind) {
    Call c = shape_call(M, N, 1, 1, kh, kh, iso);
    c.kind = kind;
    return c;
}
static PathPlan query_plan(const Call& c, long long planes, int mode, int flags, int want_hbar, int want_rho) {
    float bar = 0.f;   // (stands for a wanted gradient)
    const Grads g{nullptr, nullptr, want_hbar ? &bar : nullptr, nullptr, want_rho ? &bar : nullptr};
    PathIn q = mode == ADMM_MODE_FORWARD ? forward_in(c) : adjoint_in(c, mode == ADMM_MODE_BACKWARD ? 3 : 1, flags, g);
    q.planes = (size_t)planes;   // (given as one count, not as P x B)
    return plan_paths(q);
}

int admm_query_paths(int M, int N, int iso, int kh, long long planes, int mode, int flags, int want_hbar, int want_rho,
                     int* fwd_path, int* bwd_path) {
    if (!fwd_path || !bwd_path) return fail(ADMM_E_INVALID, "admm_query_paths: NULL output");
    if (mode != ADMM_MODE_FORWARD && mode != ADMM_MODE_RECORD && mode != ADMM_MODE_BACKWARD)
        return fail(ADMM_E_INVALID, "admm_query_paths: unknown mode %d", mode);
    const int rc = check_shape(M, N, 1, 1, kh, kh, iso);
    if (rc) return rc;
    if (planes < 0) return fail(ADMM_E_INVALID, "admm_query_paths: planes must be >= 0");
    const PathPlan pl = query_plan(query_call(M, N, iso, kh, kSingle), planes, mode, flags, want_hbar, want_rho);
    *fwd_path = pl.fwd;
    *bwd_path = pl.bwd;
    return ADMM_OK;
}

int admm_query_forward_schedule(int M, int N, int iso, int kh, long long planes, long long* chunk_planes,
                                int* streams) {
    if (!chunk_planes || !streams) return fail(ADMM_E_INVALID, "admm_query_forward_schedule: NULL output");
    const int rc = check_shape(M, N, 1, 1, kh, kh, iso);
    if (rc) return rc;
    if (planes <= 0) return fail(ADMM_E_INVALID, "admm_query_forward_schedule: planes must be > 0");
    const Call c = query_call(M, N, iso, kh, kSingle);
    const ChunkPlan cp = forward_chunks(forward_in(c), query_plan(c, planes, ADMM_MODE_FORWARD, 0, 0, 0), (size_t)planes);
    *chunk_planes = (long long)std::min(cp.chunk, (size_t)planes);
    *streams = cp.streams;
    return ADMM_OK;
}

int admm_query_grouped_path(int M, int N, int iso, int kh, long long planes, int groups, int* fwd_path) {
    if (!fwd_path) return fail(ADMM_E_INVALID, "admm_query_grouped_path: NULL output");
    const int rc = check_shape(M, N, 1, 1, kh, kh > 0 ? 1 : 0, iso);   // (kw is not given: any kw <= N)
    if (rc) return rc;
    if (planes < 0 || groups < 1 || (planes > 0 && groups > planes))
        return fail(ADMM_E_INVALID, "admm_query_grouped_path: planes must be >= 0 and 1 <= groups <= planes");
    *fwd_path = query_plan(query_call(M, N, iso, kh, kGrouped), planes, ADMM_MODE_FORWARD, 0, 0, 0).fwd;
    return ADMM_OK;
}

int admm_query_grouped_paths(int M, int N, int iso, int kh, long long planes, int groups, int mode, int flags,
                             int want_hbar, int want_rho, int* fwd_path, int* bwd_path) {
    // (the grouped sweeps form rho_bar from the same trajectory: want_rho does not change the paths)
    if (!fwd_path || !bwd_path) return fail(ADMM_E_INVALID, "admm_query_grouped_paths: NULL output");
    if (mode != ADMM_MODE_FORWARD && mode != ADMM_MODE_RECORD && mode != ADMM_MODE_BACKWARD)
        return fail(ADMM_E_INVALID, "admm_query_grouped_paths: unknown mode %d", mode);
    const int rc = check_shape(M, N, 1, 1, kh, kh > 0 ? 1 : 0, iso);   // (kw is not given: any kw <= N)
    if (rc) return rc;
    if (planes < 0 || groups < 1 || (planes > 0 && groups > planes))
        return fail(ADMM_E_INVALID, "admm_query_grouped_paths: planes must be >= 0 and 1 <= groups <= planes");
    if (mode != ADMM_MODE_FORWARD && no_plane_mode(iso, "the grouped adjoint")) return ADMM_E_UNSUPPORTED;
    const PathPlan pl = query_plan(query_call(M, N, iso, kh, kGrouped), planes, mode, flags, want_hbar, want_rho);
    *fwd_path = pl.fwd;
    *bwd_path = pl.bwd;
    return ADMM_OK;
}

int admm_query_state_path(int M, int N, int iso, int kh, long long planes, int* fwd_path) {
    if (!fwd_path) return fail(ADMM_E_INVALID, "admm_query_state_path: NULL output");
    const int rc = check_shape(M, N, 1, 1, kh, kh > 0 ? 1 : 0, iso);   // (kw is not given: any kw <= N)
    if (rc) return rc;
    if (planes < 0 || planes > (long long)kChunkPlanes)
        return fail(ADMM_E_INVALID, "admm_query_state_path: planes must be 0 .. %zu", kChunkPlanes);
    if (no_plane_mode(iso, "the state call")) return ADMM_E_UNSUPPORTED;
    *fwd_path = query_plan(query_call(M, N, iso, kh, kState), planes, ADMM_MODE_FORWARD, 0, 0, 0).fwd;
    return ADMM_OK;
}

const char* admm_path_name(int path) {
    switch (path) {
        case ADMM_PATH_FUSED: return "fused";
        case ADMM_PATH_FUSED_ISO: return "fused_iso";
        case ADMM_PATH_2PASS: return "2pass";
        case ADMM_PATH_2PASS_ISO: return "2pass_iso";
        case ADMM_PATH_RESIDENT: return "resident";
        case ADMM_PATH_SMOOTH: return "smooth";
        case ADMM_PATH_RUNTIME: return "runtime";
        case ADMM_PATH_SWEEP_FUSED: return "sweep_fused";
        case ADMM_PATH_SWEEP_FUSED_ISO: return "sweep_fused_iso";
        case ADMM_PATH_SWEEP_2PASS: return "sweep_2pass";
        case ADMM_PATH_SWEEP_2PASS_ISO: return "sweep_2pass_iso";
        case ADMM_PATH_SWEEP_RUNTIME: return "sweep_runtime";
        case ADMM_PATH_SWEEP_RUNTIME_ISO: return "sweep_runtime_iso";
        case ADMM_PATH_RESIDENT_ISO: return "resident_iso";
        default: return "none";
    }
}

}  // extern "C"
