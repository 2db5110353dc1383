"""Launches per profiler class (include/admm_deconv.h ADMM_K_*) of every call tests/test_gpu_paths.py makes, K = 4
iterations: the expected side of its exact launch-count assertions.  Recorded from the library before its launch
sequences were merged into one 2-pass forward and one reverse sweep (admm_launch.hip two_pass_forward /
two_pass_reverse), so a sequence that gains, loses or re-classes a launch on any path fails here.
For the 2-pass kernels the counts follow the sequences: forward setup 1 (one per branch in the one-grid call), prep 2
(line transform, column x conj(Sigma_c)), column K, line K - 1 (isotropic: 2 (K - 1) and norm K - 1), final 1."""

CLASSES = ("setup", "prep", "column", "line", "final", "norm", "plane", "adjoint")

# tests/paths_table.py CASES (2 planes, the plane-count rule off)
CASE_COUNTS = {
    "c2-forward": (2, 0, 0, 0, 0, 0, 1, 0),
    "c2-forward-FUSED0": (1, 2, 4, 3, 1, 0, 0, 0),
    "iso256-forward": (2, 0, 0, 0, 0, 3, 4, 0),
    "iso256-forward-FUSED0": (1, 2, 4, 6, 1, 3, 0, 0),
    "c4-forward": (1, 2, 4, 3, 1, 0, 0, 0),
    "iso512-forward": (1, 2, 4, 6, 1, 3, 0, 0),
    "250-forward": (1, 3, 0, 0, 0, 0, 1, 0),
    "240-forward": (1, 3, 0, 0, 0, 0, 1, 0),
    "96-forward": (1, 0, 0, 0, 0, 0, 1, 0),
    "250-forward-RESIDENT0": (1, 2, 4, 6, 1, 0, 0, 0),
    "250-forward-SMOOTH0": (1, 2, 4, 6, 1, 0, 0, 0),
    "250-iso-forward": (1, 3, 0, 0, 0, 3, 4, 0),
    "250-iso-forward-RESIDENT0": (1, 2, 4, 9, 1, 3, 0, 0),
    "480x640-forward": (1, 2, 4, 6, 1, 0, 0, 0),
    "primes-forward": (1, 2, 4, 6, 1, 0, 0, 0),
    "128-forward": (1, 3, 0, 0, 0, 0, 1, 0),
    "128-forward-RESIDENT0": (1, 2, 4, 3, 1, 0, 0, 0),
    "96-iso-forward": (1, 0, 0, 0, 0, 3, 4, 0),
    "32-iso-forward": (1, 3, 0, 0, 0, 3, 4, 0),
    "128-forward-RESIDENT2": (1, 3, 0, 0, 0, 0, 1, 0),
    "demo32-record-RESIDENT2": (1, 4, 4, 0, 5, 0, 1, 4),
    "demo32-record-hbar-RESIDENT2": (1, 3, 8, 3, 10, 0, 0, 4),
    "64-iso-RESIDENT2": (1, 0, 0, 0, 0, 3, 4, 0),
    "250-iso-RESIDENT2": (1, 3, 0, 0, 0, 3, 4, 0),
    "250-iso-record-RESIDENT2": (1, 4, 4, 4, 5, 6, 4, 7),
    "128-iso-backward-RESIDENT2": (1, 1, 4, 0, 2, 6, 4, 7),
    "128-iso-backward-hbar-RESIDENT2": (1, 3, 8, 6, 10, 6, 0, 7),
    "c5-record-masks": (2, 0, 0, 0, 2, 0, 1, 1),
    "c5-record-full": (2, 1, 0, 0, 2, 0, 1, 1),
    "c5-record-FUSED_ADJ0": (2, 1, 4, 0, 2, 0, 1, 4),
    "c5iso-record-masks": (2, 0, 0, 0, 2, 6, 4, 4),
    "c5iso-record-full": (1, 3, 8, 6, 3, 6, 0, 7),
    "256-record-hbar": (1, 3, 8, 3, 10, 0, 0, 4),
    "256-record-hbar-masks": (1, 3, 8, 3, 10, 0, 0, 4),
    "256-backward-norho": (2, 0, 0, 0, 5, 0, 1, 1),
    "256-backward-rho": (2, 1, 0, 0, 5, 0, 1, 1),
    "256-backward-hbar": (1, 3, 8, 3, 10, 0, 0, 4),
    "iso256-backward-norho": (2, 0, 0, 0, 5, 6, 4, 4),
    "iso256-backward-rho": (1, 3, 8, 6, 6, 6, 0, 7),
    "c4-backward": (1, 3, 8, 3, 10, 0, 0, 4),
    "250-record": (1, 4, 4, 4, 5, 0, 1, 4),
    "250-record-hbar": (1, 3, 8, 10, 10, 0, 0, 4),
    "250-iso-backward": (1, 3, 8, 13, 10, 6, 0, 7),
    "primes-backward": (1, 3, 8, 10, 10, 0, 0, 4),
}

# tests/paths_table.py PLANE_CASES (the row's plane count, the library's default rule)
PLANE_COUNTS = {
    "c2-95": (1, 2, 4, 3, 1, 0, 0, 0),
    "c2-96": (2, 0, 0, 0, 0, 0, 1, 0),
    "c5-record-masks-64": (1, 3, 8, 3, 3, 0, 0, 4),
    "c5-record-masks-96": (2, 0, 0, 0, 2, 0, 1, 1),
    "256-backward-norho-8": (1, 3, 8, 3, 6, 0, 0, 4),
    "iso256-forward-111": (1, 2, 4, 6, 1, 3, 0, 0),
    "iso256-forward-112": (2, 0, 0, 0, 0, 3, 4, 0),
    "c5iso-record-masks-6": (1, 3, 8, 6, 3, 6, 0, 7),
    "c5iso-record-masks-128": (2, 0, 0, 0, 2, 6, 4, 4),
    "250-forward-128": (1, 2, 4, 6, 1, 0, 0, 0),
    "250-forward-192": (1, 3, 0, 0, 0, 0, 1, 0),
    "250-record-64": (1, 3, 8, 10, 6, 0, 0, 4),
    "128-forward-191": (1, 2, 4, 3, 1, 0, 0, 0),
    "128-forward-192": (1, 3, 0, 0, 0, 0, 1, 0),
    "96-forward-6": (1, 0, 0, 0, 0, 0, 1, 0),
    "32-demo-forward-6": (1, 3, 0, 0, 0, 0, 1, 0),
    "96-iso-forward-255": (1, 2, 4, 9, 1, 3, 0, 0),
    "96-iso-forward-256": (1, 0, 0, 0, 0, 3, 4, 0),
    "250-iso-forward-255": (1, 2, 4, 9, 1, 3, 0, 0),
    "250-iso-forward-256": (1, 3, 0, 0, 0, 3, 4, 0),
    "32-iso-forward-6": (1, 2, 4, 6, 1, 3, 0, 0),
}

# the one-grid multi-branch call at 256 x 256, 2 branches, B = 1, P = 1: (isotropic, default plane-count rule) ->
# (the recording forward alone, forward + recorded backward); with the rule the 2-pass grid, without it the fused one
MULTI_COUNTS = {
    (False, True): ((2, 2, 4, 3, 1, 0, 0, 0), (2, 3, 8, 3, 6, 0, 0, 4)),
    (False, False): ((4, 0, 0, 0, 0, 0, 1, 0), (4, 1, 0, 0, 5, 0, 1, 1)),
    (True, True): ((2, 2, 4, 6, 1, 3, 0, 0), (2, 3, 8, 6, 6, 6, 0, 7)),
    (True, False): ((4, 0, 0, 0, 0, 3, 4, 0), (4, 0, 0, 0, 5, 6, 4, 4)),
}

# the grouped adjoint (tests/test_gpu_grouped_adjoint.py grouped_launch_counts: K = 4, B = 2, P = 3, a group per plane,
# 5 x 5 PSFs, the plane-count rule off): "MxN-prox-call-variant", call = record + replay counted together or the
# combined call, variant = with h_bar ("h"), without ("noh"), or y_bar and rho_bar not asked for ("drop").
# Recorded from commit 743899b, before the single and the grouped adjoint driver were merged into one
# (admm_launch.hip launch_backward).
GROUPED_COUNTS = {
    "32x32-aniso-replay-h": (1, 3, 8, 3, 10, 0, 0, 4),
    "32x32-aniso-replay-noh": (1, 3, 8, 3, 6, 0, 0, 4),
    "32x32-aniso-replay-drop": (1, 3, 8, 3, 7, 0, 0, 4),
    "32x32-aniso-combined-h": (1, 3, 8, 3, 10, 0, 0, 4),
    "32x32-aniso-combined-noh": (1, 3, 8, 3, 6, 0, 0, 4),
    "32x32-aniso-combined-drop": (1, 3, 8, 3, 7, 0, 0, 4),
    "32x32-iso-replay-h": (1, 3, 8, 6, 10, 6, 0, 7),
    "32x32-iso-replay-noh": (1, 3, 8, 6, 6, 6, 0, 7),
    "32x32-iso-replay-drop": (1, 3, 8, 6, 7, 6, 0, 7),
    "32x32-iso-combined-h": (1, 3, 8, 6, 10, 6, 0, 7),
    "32x32-iso-combined-noh": (1, 3, 8, 6, 6, 6, 0, 7),
    "32x32-iso-combined-drop": (1, 3, 8, 6, 7, 6, 0, 7),
    "24x20-aniso-replay-h": (1, 3, 8, 10, 10, 0, 0, 4),
    "24x20-aniso-replay-noh": (1, 3, 8, 10, 6, 0, 0, 4),
    "24x20-aniso-replay-drop": (1, 3, 8, 10, 7, 0, 0, 4),
    "24x20-aniso-combined-h": (1, 3, 8, 10, 10, 0, 0, 4),
    "24x20-aniso-combined-noh": (1, 3, 8, 10, 6, 0, 0, 4),
    "24x20-aniso-combined-drop": (1, 3, 8, 10, 7, 0, 0, 4),
    "24x20-iso-replay-h": (1, 3, 8, 13, 10, 6, 0, 7),
    "24x20-iso-replay-noh": (1, 3, 8, 13, 6, 6, 0, 7),
    "24x20-iso-replay-drop": (1, 3, 8, 13, 7, 6, 0, 7),
    "24x20-iso-combined-h": (1, 3, 8, 13, 10, 6, 0, 7),
    "24x20-iso-combined-noh": (1, 3, 8, 13, 6, 6, 0, 7),
    "24x20-iso-combined-drop": (1, 3, 8, 13, 7, 6, 0, 7),
    "256x256-aniso-replay-noh": (2, 1, 4, 0, 5, 0, 1, 4),
    "256x256-aniso-replay-drop": (2, 1, 4, 0, 2, 0, 1, 4),
    "256x256-aniso-combined-noh": (2, 1, 4, 0, 5, 0, 1, 4),
    "256x256-aniso-combined-drop": (2, 1, 4, 0, 2, 0, 1, 4),
}
