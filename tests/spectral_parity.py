"""Per-bin parity on flat-spectrum inputs, and the cases of the FFT length sweep (DESIGN.md s2 "Length sweep").

tests/parity.py bounds the error of a whole plane (rel-L2, max-abs) on synth images, whose energy sits in a few low bins:
a bin that is 100 % wrong away from them passes.  Here the inputs are white noise, so every bin of the solve carries
signal, and the figure is per bin:

    bin_error(got, ref) = max over bins |FFT2(got - ref)| / rms over bins |FFT2(ref)|      (worst plane, numpy fp64)

The yardstick of a case is e = bin_error of the fp64 oracle's own float32 evaluation (tests/state_oracle.py: the same
loop rounded to float32 after every operator, numpy's transforms) against the fp64 oracle; the library's figure g is
bounded by c_f * e with one constant per kernel family f (BOUND_FACTOR), times sqrt(R / 7) where the runtime plan has a
direct-DFT factor R (a sum of R rounded terms random-walks).  c_f = 4 x the family's median g / e on the MI355X run
logged in profiles/length_sweep_parity.jsonl."""
import collections
import functools
import math

import numpy as np

import state_oracle as so
from admm_deconv import synth

LAM, RHO, K = 0.05, 0.1, 3

# admm_smooth.hip SM_LENGTHS / SM_COL_ASC_LENGTHS (tests/test_spectral_parity.py keeps them in step with the source)
COMPILED_LENGTHS = (64, 96, 100, 120, 128, 144, 160, 192, 200, 240, 250, 256, 288, 300, 320, 360, 384, 400, 480, 500, 512,
                    576, 600, 640, 720, 768, 800, 960, 1000, 1024, 1080, 1200, 1280, 1440, 1536, 1920, 2000, 2048, 2560,
                    3000, 4096)
COL_ASC_LENGTHS = (192, 200, 250, 300, 320, 360, 400, 500, 600, 720, 1200, 2000)

# runtime plans (admm_launch.hip make_fplan): radices 8 / 4 / 2 / 3 / 5 in registers, a direct DFT per other prime
RUNTIME_LENGTHS = (
    2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 16, 24, 32, 40, 56, 64,   # single radices and pairs
    49, 121, 125, 243, 343, 2187, 2401, 3125,                            # prime powers
    77, 91, 143, 221, 323,                                               # two direct-DFT factors
    127, 251, 257, 509, 1021, 2039,                                      # primes: one lane runs the whole R^2 DFT
    3072, 3993, 4000, 4094, 4095, 4096,                                  # near the top
)
ISO_COMPILED = (96, 250, 1000, 4096)
ISO_RUNTIME = (7, 77, 243, 251)
ADJOINT_LENGTHS = (49, 77, 243, 251, 1000, 4095)

LINE_N = 9    # line role: 9 lines of L pixels -- odd, so the last line of a real-pair transform is unpaired, and the
              # runtime line blocks (gen_T: 8 lines to L = 256, 2 to 1024, then 1) end in a ragged 1-line block
COL_M = 18    # column role: L lines of 18 pixels -- H = 10 bins; gen_KB leaves a ragged last block from N = 128

# c_f: 4 x the family's median g / e of profiles/length_sweep_parity.jsonl, rounded down (module docstring)
#      medians there: compiled line 1.50, compiled column 1.51, runtime 2-3-5-smooth 1.33, runtime with a direct DFT 1.69
BOUND_FACTOR = {"compiled_line": 6.0, "compiled_column": 6.05, "runtime_smooth": 5.3, "runtime_direct": 6.75}

Case = collections.namedtuple("Case", "id role L N M B iso smooth path family R seed")


def factors(n):
    """make_fplan's factorisation of a runtime length, in its order."""
    r, m = [], n
    while m % 8 == 0:
        r.append(8); m //= 8
    for f in (4, 2):
        if m % f == 0:
            r.append(f); m //= f
    for f in (3, 5):
        while m % f == 0:
            r.append(f); m //= f
    f = 7
    while f * f <= m:
        while m % f == 0:
            r.append(f); m //= f
        f += 2
    if m > 1:
        r.append(m)
    assert math.prod(r) == n
    return r


def direct_factor(n):
    """The largest factor of n that the runtime plan evaluates as a direct DFT (0: none)."""
    return max([f for f in factors(n) if f not in (8, 4, 2, 3, 5)], default=0)


# Seeds replaced on the CPU (tests/test_spectral_parity.py: a case that misses a check there gets another seed, never on
# the GPU).  Adjoint cases: the first seed whose oracle |s_k| all stay 1e-5 from tau (at 4095 x 18 one seed in ~2000
# does).  2039 x 18: at R = 2039 the sqrt(R / 7) allowance puts the bound at the size of a 1e-3 single-bin error, and
# the teeth hold by the seed only (DESIGN.md s2 "Length sweep").
SEEDS = {"column-2039x18": 2139018, "column-49x18-adj": 149018, "line-9x243-adj": 109243, "column-243x18-adj": 443018,
         "line-9x1000-adj": 210000, "column-1000x18-adj": 2900018, "line-9x4095-adj": 18413095,
         "column-4095x18-adj": 699595018}


def _case(role, L, B=2, iso=False, smooth=None, tag=""):
    """smooth: the SMOOTH option of the call (None: the default, 1); 0 runs a compiled length through a runtime plan."""
    N, M = (LINE_N, L) if role == "line" else (L, COL_M)
    compiled = L in COMPILED_LENGTHS and smooth != 0
    R = 0 if compiled else direct_factor(L)
    family = f"compiled_{role}" if compiled else ("runtime_direct" if R else "runtime_smooth")
    cid = f"{role}-{N}x{M}" + ("-iso" if iso else "") + tag
    return Case(cid, role, L, N, M, B, iso, smooth, "smooth" if compiled else "runtime", family, R,
                SEEDS.get(cid, 1000 * N + M + (7 if iso else 0)))


def compiled_cases():
    out = []
    for L in COMPILED_LENGTHS:
        asc = L in COL_ASC_LENGTHS
        out.append(_case("line", L))
        out.append(_case("column", L, tag="-asc" if asc else "-desc"))
        out.append(_case("column", L, smooth=3 if asc else 2, tag="-desc-forced" if asc else "-asc-forced"))
    return out


def runtime_cases():
    return [_case(role, L, smooth=0 if L in COMPILED_LENGTHS else None, tag="-rt" if L in COMPILED_LENGTHS else "")
            for L in RUNTIME_LENGTHS for role in ("line", "column")]


def iso_cases():
    return [_case(role, L, B=3, iso=True) for L in ISO_COMPILED + ISO_RUNTIME for role in ("line", "column")]


def adjoint_cases():
    return [_case(role, L, tag="-adj") for L in ADJOINT_LENGTHS for role in ("line", "column")]


def forward_cases():
    return compiled_cases() + runtime_cases() + iso_cases()


def white_case(N, M, B, P, seed):
    """(y, lambda, rho, psf): y (B, P, N, M) standard normal float32; a 3 x 3 PSF where both sides hold it."""
    y = np.random.default_rng(seed).standard_normal((B, P, N, M)).astype(np.float32)
    return y, LAM, RHO, synth.gaussian_psf(3, 0.8) if min(N, M) >= 3 else None


def inputs(case):
    return white_case(case.N, case.M, case.B, 1, case.seed)


@functools.lru_cache(maxsize=None)
def _oracle(N, M, B, iso, seed, k):
    y, lam, rho, h = white_case(N, M, B, 1, seed)
    return so.solve(y, lam, rho, h, iso, k), so.solve(y, lam, rho, h, iso, k, dtype=np.float32)


def oracle(case, k=K):
    """(fp64 oracle, its float32 evaluation) of `k` iterations: computed once per input, shared, never modified."""
    return _oracle(case.N, case.M, case.B, case.iso, case.seed, k)


def prox_fraction(case):
    """Mean fraction of live prox outputs over the iterations that reach x_K (1 .. K - 1)."""
    return float(np.mean(oracle(case)[0]["prox_active"][:K - 1]))


def threshold_margin(case):
    """Smallest | |s_k| - tau | of the fp64 oracle over k = 1 .. K - 1: how far its prox masks are from flipping."""
    tau = float(np.float32(LAM)) / float(np.float32(RHO))
    return min(float(np.abs(np.abs(oracle(case, k)[0]["state"]) - tau).min()) for k in range(1, K))


def bin_error(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    g = got.reshape(-1, *got.shape[-2:])
    r = ref.reshape(-1, *ref.shape[-2:])
    worst = 0.0
    for i in range(g.shape[0]):
        R = np.abs(np.fft.fft2(r[i]))
        worst = max(worst, float(np.abs(np.fft.fft2(g[i] - r[i])).max() / np.sqrt(np.mean(R * R))))
    return worst


def yardstick(case):
    r64, r32 = oracle(case)
    return bin_error(r32["x"], r64["x"])


def bound(case):
    """c_f * e (* sqrt(R / 7) with a direct-DFT factor R) -- the per-bin bound of a case (module docstring)."""
    return BOUND_FACTOR[case.family] * yardstick(case) * (math.sqrt(case.R / 7.0) if case.R else 1.0)


def mutate_bin(x, j, k, rel=1e-3):
    """x (..., N, M) with a relative error `rel` in bin (j, k) of every plane's 2-D spectrum, and in its mirror."""
    X = np.fft.fft2(np.asarray(x, np.float64))
    N, M = X.shape[-2:]
    X[..., j, k] *= 1.0 + rel
    if ((-j) % N, (-k) % M) != (j, k):
        X[..., (-j) % N, (-k) % M] *= 1.0 + rel
    return np.real(np.fft.ifft2(X))
