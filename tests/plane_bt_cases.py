"""The cases of the per-plane isotropic mode's tests (CPU: tests/test_plane_bt.py, GPU: tests/test_gpu_plane_bt.py).

White noise (plane_bt_oracle.inputs), lambda 0.05, rho 0.1 (tau = 0.5), Gaussian k x k PSF of sigma 1.  A case is
(B, P, N, M, k): N lines of M pixels.  Forward K = 6 (256 x 256: K = 3), adjoint K = 4."""

FWD_SEED = 7
K_FWD, K_ADJ = 6, 4

# the tuned power-of-two shapes: the 2-pass grid
FWD_2PASS = [
    (2, 1, 8, 16, 0),      # one line block whose halo wraps onto itself
    (2, 3, 16, 32, 5),     # two blocks
    (1, 2, 16, 512, 3),    # 512-point lines: the 8-line / 512-thread / just-in-time form
    (1, 2, 8, 1024, 0),    # T = 4
    (2, 1, 2, 4, 0),       # the smallest shape
    (1, 2, 256, 256, 15),  # K = 3: the shape whose anisotropic twin goes fused, here 2-pass
]
# every other shape: the runtime-length kernels
FWD_RUNTIME = [
    (2, 2, 9, 10, 3),      # a ragged last block
    (2, 3, 30, 40, 5),
    (2, 1, 7, 33, 0),      # odd M, a direct-DFT factor
    (1, 2, 3, 2000, 3),    # one or two long lines per block
    (1, 2, 250, 18, 3),    # a smooth length that must stay on the runtime kernels
]
FWD_CASES = FWD_2PASS + FWD_RUNTIME


def fwd_K(case):
    return 3 if case[2:4] == (256, 256) else K_FWD


# adjoint: (case, seed) -- the seed keeps every |s_k| at least 1e-5 from tau in the fp64 oracle (asserted on the CPU)
ADJ_CASES = [
    ((2, 3, 16, 32, 5), 7),
    ((2, 1, 8, 16, 0), 8),
    ((1, 2, 16, 512, 3), 8),
    ((2, 2, 9, 10, 3), 7),
    ((2, 3, 30, 40, 5), 7),
    ((1, 2, 3, 2000, 3), 7),
]


def case_id(c):
    return "x".join(str(v) for v in c[:4]) + f"-k{c[4]}"
