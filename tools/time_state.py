"""Time the resumable solve at c2 (512 x 256^2, 15x15 PSF, K = 25, anisotropic; the fused path) against the plain solve.

  python tools/time_state.py [--parent-tree DIR] [NAME=VALUE library options]
(DIR: a checkout of the parent commit with its library built)

Measures, each as the median of WINDOWS windows of REPS calls between device events (after warm-up):
  plain          tvd_fft of this tree -- and, with --parent-tree, of the parent commit's package and library: two runs
                 of each, alternating, every run a fresh child process (so each loads one library only)
  state_cold     tvd_fft_state from the zero state with state and residuals out
  state_cold_x   the same with neither (the pass-through call: the state instance's stored s_{K-1} only)
  state_warm     the continuation call (state in, state and residuals out)
  kernels        the start / end kernels alone, from the library profiler's classes on an instrumented call:
                 v0 (PREP of the warm call), import (PLANE warm - PLANE cold), end (FINAL without residuals),
                 resid (FINAL with - FINAL without)
  tol            tvd_fft_tol (eps_rel 1e-2, check_every 10, maxit 100) against tvd_fft at maxit = 100
and the byte model of DESIGN.md (B/px over the plain call's 476).  Writes $OUT_DIR/state_c2.json
(default bench_out/)."""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
# ADMM_TREE: the checkout whose package and library a --plain-only child times (default: this tree)
sys.path.insert(0, os.path.join(os.environ.get("ADMM_TREE") or os.path.join(HERE, ".."), "admm-deconv_amd"))

WINDOWS, REPS, WARM = 7, 5, 3
M = N = 256
B, K, PSF = 512, 25, (15, 2.5)


def timed(fn):
    """median ms per call over WINDOWS windows of REPS calls, and the windows' spread (max - min) / median"""
    import torch
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / REPS)
    med = statistics.median(ms)
    return {"ms": round(med, 4), "spread": round((max(ms) - min(ms)) / med, 4)}


def setup():
    import torch
    import admm_deconv
    from admm_deconv import synth
    dev = torch.device("cuda", 0)
    psf = synth.gaussian_psf(*PSF)
    y = torch.from_numpy(synth.make_batch(8, M, N, psf)).to(dev).repeat(B // 8, 1, 1, 1).contiguous()
    one = lambda v: torch.tensor([v], dtype=torch.float32, device=dev)   # noqa: E731
    return admm_deconv, y, one(synth.LAMBDA), one(synth.RHO), torch.from_numpy(psf).to(dev)


def plain_only():
    ad, y, lam, rho, h = setup()
    print(json.dumps(timed(lambda: ad.tvd_fft(y, lam, rho, h, False, K))))


def child_plain(tree):
    env = dict(os.environ)
    env.pop("ADMM_TREE", None)
    if tree:
        env["ADMM_TREE"] = os.path.abspath(tree)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only"], env=env, capture_output=True, text=True,
                       timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f"plain run failed ({tree or 'this tree'}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def profile_classes(fn):
    from admm_deconv import _lib
    _lib.profile_reset()
    _lib.profile_enable(True)
    fn()
    _lib.profile_enable(False)
    out = {}
    for cls, name in _lib.KERNEL_CLASSES.items():
        ms, n = _lib.profile_get(cls)
        if n:
            out[name] = round(ms, 4)
    return out


def main():
    args = sys.argv[1:]
    if "--plain-only" in args:
        return plain_only()
    parent = args[args.index("--parent-tree") + 1] if "--parent-tree" in args else None
    res = {"config": {"M": M, "N": N, "B": B, "K": K, "psf": list(PSF), "windows": WINDOWS, "reps": REPS}}
    # the plain call, every run its own process: parent, tree, parent, tree
    res["plain_tree"], res["plain_parent"] = [], []
    for _ in range(2):
        if parent:
            res["plain_parent"].append(child_plain(parent))
        res["plain_tree"].append(child_plain(None))
    ad, y, lam, rho, h = setup()
    from admm_deconv import _lib
    for a in [a for a in args if "=" in a]:
        _lib.set_option(a.split("=")[0].upper(), int(a.split("=")[1]))
    res["path"] = _lib.query_state_path(M, N, False, PSF[0], B)
    res["plain"] = timed(lambda: ad.tvd_fft(y, lam, rho, h, False, K))
    res["state_cold"] = timed(lambda: ad.tvd_fft_state(y, lam, rho, h, False, K))
    res["state_cold_x"] = timed(lambda: ad.tvd_fft_state(y, lam, rho, h, False, K, want_state=False, want_residuals=False))
    _, s0, _ = ad.tvd_fft_state(y, lam, rho, h, False, K, want_residuals=False)
    res["state_warm"] = timed(lambda: ad.tvd_fft_state(y, lam, rho, h, False, K, state=s0))
    cold = profile_classes(lambda: ad.tvd_fft_state(y, lam, rho, h, False, K))
    cold_ns = profile_classes(lambda: ad.tvd_fft_state(y, lam, rho, h, False, K, want_residuals=False))
    warm = profile_classes(lambda: ad.tvd_fft_state(y, lam, rho, h, False, K, state=s0))
    res["classes"] = {"cold": cold, "cold_no_resid": cold_ns, "warm": warm}
    res["kernels_ms"] = {"v0": warm.get("prep"), "import": round(warm["plane"] - cold["plane"], 4),
                         "end": cold_ns.get("final"), "resid": round(cold["final"] - cold_ns["final"], 4),
                         "plane_cold": cold["plane"]}
    # bytes per pixel: the plain call, the stored s_{K-1}, the end kernel (x 4, s_{K-1} 8, s_K 8), the residual pass
    # (s_{K-1} rewritten in the natural layout 8, s_K and s_{K-1} read 16), the warm start (import 16, v_0 kernel 12,
    # v_0 and s_0 read by the solve 12)
    model = {"plain": 476, "s_prev_stored": 8, "end": 20, "resid": 24, "warm": 40}
    res["byte_model"] = model
    res["ratios"] = {"cold_measured": round(res["state_cold"]["ms"] / res["plain"]["ms"], 4),
                     "cold_model": round((476 + 8 + 20 + 24) / 476, 4),
                     "warm_measured": round(res["state_warm"]["ms"] / res["plain"]["ms"], 4),
                     "warm_model": round((476 + 8 + 20 + 24 + 40) / 476, 4)}
    import time
    import torch

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, 1000 * (time.perf_counter() - t0)
    (_, _, iters, _), tol_ms = wall(lambda: ad.tvd_fft_tol(y, lam, rho, h, False, 100, eps_rel=1e-2, check_every=10))
    _, full_ms = wall(lambda: ad.tvd_fft(y, lam, rho, h, False, 100))
    res["tol"] = {"iters": iters, "ms": round(tol_ms, 3), "maxit100_ms": round(full_ms, 3), "eps_rel": 1e-2, "check_every": 10}
    print(json.dumps(res))
    out = os.environ.get("OUT_DIR", "bench_out")
    os.makedirs(out, exist_ok=True)
    json.dump(res, open(os.path.join(out, "state_c2.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
