/* Host-side AddressSanitizer check of the resumable solve's C ABI (admm_tvd_state_workspace_bytes,
 * admm_tvd_forward_state_dev_f32, admm_query_state_path).
 *
 * Built by __graft_entry__.build_asan() against libadmm_deconv_asan.so exactly like capi_host_check.c: the library's
 * host code instrumented, device code untouched.  Runs WITHOUT a GPU: the workspace layout over a sweep of shapes, the
 * state call's argument validation (every refusal comes before the first launch) and the path query.  Exits 0 if every
 * call returned what the header promises; ASan aborts on any out-of-bounds access, use-after-free or leak in that host
 * code.  tests/test_asan_state.py runs it. */
#include <stdio.h>
#include <string.h>

#include "admm_deconv.h"

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

static void sizes(void) {
    static const int shapes[][2] = {{2, 2},     {3, 5},     {16, 8},    {64, 64},   {96, 96},     {250, 250}, {256, 256},
                                    {480, 640}, {512, 512}, {37, 29},   {1024, 16}, {2048, 2048}, {4096, 2}};
    for (size_t i = 0; i < sizeof(shapes) / sizeof(shapes[0]); ++i) {
        for (int iso = 0; iso < 2; ++iso) {
            for (int k = 0; k < 3; ++k) {
                const int M = shapes[i][0], N = shapes[i][1];
                const int kh = k == 0 ? 0 : (k == 1 ? 1 : (M < 15 ? M : 15));
                const int kw = k == 0 ? 0 : (k == 1 ? 1 : (N < 10 ? N : 10));
                size_t fw = 0, sw = 0, one = 0;
                CHECK(admm_tvd_workspace_bytes(M, N, 3, 5, kh, kw, iso, &fw) == ADMM_OK);
                CHECK(admm_tvd_state_workspace_bytes(M, N, 3, 5, kh, kw, iso, &sw) == ADMM_OK);
                CHECK(admm_tvd_state_workspace_bytes(M, N, 1, 1, kh, kw, iso, &one) == ADMM_OK);
                CHECK(sw >= fw && sw % 256 == 0 && one % 256 == 0 && one < sw);
                CHECK(sw >= fw + (size_t)15 * M * N * 4 || sw >= (size_t)15 * M * N * 4 * 5);
            }
        }
    }
    size_t w = 0;
    CHECK(admm_tvd_state_workspace_bytes(8, 8, 1, 65280, 3, 3, 0, &w) == ADMM_OK && w > 0);
    CHECK(admm_tvd_state_workspace_bytes(8, 8, 1, 65281, 3, 3, 0, &w) == ADMM_E_UNSUPPORTED);
    CHECK(admm_tvd_state_workspace_bytes(8, 8, 255, 257, 3, 3, 1, &w) == ADMM_E_UNSUPPORTED);
    CHECK(admm_tvd_state_workspace_bytes(64, 64, 1, 2, 5, 5, 0, NULL) == ADMM_E_INVALID);
    CHECK(admm_tvd_state_workspace_bytes(1, 64, 1, 2, 0, 0, 0, &w) == ADMM_E_UNSUPPORTED);
    CHECK(admm_tvd_state_workspace_bytes(64, 4097, 1, 2, 0, 0, 0, &w) == ADMM_E_UNSUPPORTED);
    CHECK(admm_tvd_state_workspace_bytes(64, 64, 0, 2, 0, 0, 0, &w) == ADMM_E_INVALID);
    CHECK(admm_tvd_state_workspace_bytes(64, 64, 1, 2, 5, 0, 0, &w) == ADMM_E_INVALID);
    CHECK(admm_tvd_state_workspace_bytes(64, 64, 1, 2, 65, 5, 0, &w) == ADMM_E_UNSUPPORTED);
}

/* "device pointers" that are never dereferenced: every call below is refused before the first launch */
static float* const P0 = (float*)(size_t)(1 << 20);
static float* const P1 = (float*)(size_t)(2 << 20);
static float* const P2 = (float*)(size_t)(3 << 20);
static void* const WS = (void*)(size_t)(16 << 20);

static int call(int M, int N, int P, int B, const float* h, int kh, int kw, const float* lam, const float* rho, int iso,
                int maxit, const float* s_in, float* s_out, void* ws, size_t ws_bytes) {
    return admm_tvd_forward_state_dev_f32(P0, P1, M, N, P, B, h, kh, kw, lam, rho, iso, maxit, s_in, s_out, NULL, ws,
                                          ws_bytes, NULL);
}

static void refusals(void) {
    const size_t big = (size_t)1 << 40;
    CHECK(call(64, 32, 3, 2, P2, 5, 5, P2, P2, 0, 0, NULL, NULL, WS, big) == ADMM_E_INVALID);
    CHECK(strstr(admm_last_error(), "maxit") != NULL);
    CHECK(call(64, 32, 3, 2, P2, 5, 5, P2, P2, 0, -3, NULL, NULL, WS, big) == ADMM_E_INVALID);
    CHECK(call(64, 32, 3, 2, P2, 5, 5, P2, P2, 0, 5, P2, P2, WS, big) == ADMM_E_INVALID);
    CHECK(strstr(admm_last_error(), "state_out") != NULL);
    CHECK(call(64, 32, 3, 2, P2, 5, 5, NULL, P2, 0, 5, NULL, NULL, WS, big) == ADMM_E_INVALID);
    CHECK(call(64, 32, 3, 2, P2, 5, 5, P2, NULL, 1, 5, NULL, NULL, WS, big) == ADMM_E_INVALID);
    CHECK(call(64, 32, 3, 2, NULL, 5, 5, P2, P2, 0, 5, NULL, NULL, WS, big) == ADMM_E_INVALID);
    CHECK(call(8, 8, 1, 65281, NULL, 0, 0, P2, P2, 0, 5, NULL, NULL, WS, big) == ADMM_E_UNSUPPORTED);
    CHECK(call(1, 32, 3, 2, NULL, 0, 0, P2, P2, 0, 5, NULL, NULL, WS, big) == ADMM_E_UNSUPPORTED);
    CHECK(call(64, 4097, 3, 2, NULL, 0, 0, P2, P2, 0, 5, NULL, NULL, WS, big) == ADMM_E_UNSUPPORTED);
    CHECK(call(64, 32, 3, 2, NULL, 0, 0, P2, P2, 0, 5, P2 + 1, NULL, WS, big) == ADMM_E_INVALID);
    size_t fw = 0, sw = 0;
    CHECK(admm_tvd_workspace_bytes(64, 32, 3, 2, 5, 5, 1, &fw) == ADMM_OK);
    CHECK(admm_tvd_state_workspace_bytes(64, 32, 3, 2, 5, 5, 1, &sw) == ADMM_OK);
    CHECK(call(64, 32, 3, 2, P2, 5, 5, P2, P2, 1, 5, NULL, NULL, WS, fw) == ADMM_E_WORKSPACE);
    CHECK(call(64, 32, 3, 2, P2, 5, 5, P2, P2, 1, 5, NULL, NULL, WS, sw - 1) == ADMM_E_WORKSPACE);
    CHECK(call(64, 32, 3, 2, P2, 5, 5, P2, P2, 1, 5, NULL, NULL, (char*)WS + 64, big) == ADMM_E_WORKSPACE);
    CHECK(call(64, 32, 3, 2, P2, 5, 5, P2, P2, 1, 5, NULL, NULL, NULL, big) == ADMM_E_WORKSPACE);
    CHECK(strlen(admm_last_error()) > 0);
}

static int path(int M, int N, int iso, int kh, long long planes) {
    int f = -1;
    return admm_query_state_path(M, N, iso, kh, planes, &f) == ADMM_OK ? f : -1;
}

static void paths(void) {
    CHECK(path(256, 256, 0, 15, 512) == ADMM_PATH_FUSED);
    CHECK(path(256, 256, 0, 15, 8) == ADMM_PATH_2PASS);
    CHECK(path(256, 256, 1, 15, 512) == ADMM_PATH_2PASS_ISO);
    CHECK(path(64, 64, 0, 9, 2) == ADMM_PATH_2PASS);
    CHECK(path(96, 96, 0, 9, 512) == ADMM_PATH_RUNTIME);
    CHECK(path(250, 250, 1, 9, 512) == ADMM_PATH_RUNTIME);
    CHECK(path(40, 30, 0, 0, 1) == ADMM_PATH_RUNTIME);
    CHECK(admm_set_option(ADMM_OPT_FUSED, 0) == ADMM_OK);
    CHECK(path(256, 256, 0, 15, 512) == ADMM_PATH_2PASS);
    CHECK(admm_set_option(ADMM_OPT_FUSED, 1) == ADMM_OK);
    int f = 0;
    CHECK(admm_query_state_path(256, 256, 0, 15, 512, NULL) == ADMM_E_INVALID);
    CHECK(admm_query_state_path(256, 256, 0, 15, -1, &f) == ADMM_E_INVALID);
    CHECK(admm_query_state_path(256, 256, 0, 15, 65281, &f) == ADMM_E_INVALID);
    CHECK(admm_query_state_path(4097, 256, 0, 0, 4, &f) == ADMM_E_UNSUPPORTED);
}

int main(void) {
    sizes();
    refusals();
    paths();
    if (failures) {
        fprintf(stderr, "asan state host check: %d failure(s)\n", failures);
        return 1;
    }
    printf("asan state host check: ok\n");
    return 0;
}
