"""Time the grouped solve on c2's workload with one PSF per image: 512 x 256^2, 15 x 15 Gaussian PSFs with sigma spread
over 1.0 .. 3.0 (G = 512), K = 25, lambda 0.0041, rho 0.021 (DESIGN.md s5 "Grouped solve").

Modes (one JSON line each; hipEvent timing, warm-up, median over the steps):
  grouped  one tvd_fft_grouped call
  loop     what users did before: 512 single-image tvd_fft calls, each with its own PSF
  ceiling  one single-PSF tvd_fft call over the same batch (every plane shares one table set)
Training-step modes (a recorded forward and its reverse sweep with y_bar, h_bar, lambda_bar and rho_bar; x_bar = x - y):
  train          one tvd_fft_grouped_record + tvd_fft_grouped_backward_recorded
  train_loop     what users did before: 512 single-image tvd_fft_record + tvd_fft_backward_recorded calls
  train_ceiling  one single-PSF tvd_fft_record + tvd_fft_backward_recorded over the same batch
--profile: after timing a mode, one more call under the library profiler; its per-class milliseconds go into the line.
--pkg DIR: import admm_deconv from another build of the package (e.g. the parent commit's, which has no grouped
entry: modes loop and ceiling).  usage: bench_grouped.py [--modes grouped,loop,ceiling] [--steps 20] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--modes", default="grouped,loop,ceiling")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--maxit", type=int, default=25)
ap.add_argument("--pkg", default=os.path.join(REPO, "admm-deconv_amd"))
ap.add_argument("--tag", default="branch")
ap.add_argument("--profile", action="store_true")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.pkg))
import admm_deconv  # noqa: E402
from admm_deconv import synth  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_grouped: no GPU (there is no CPU path)")
dev = torch.device("cuda", 0)
B, K, LAM, RHO = args.batch, args.maxit, synth.LAMBDA, synth.RHO
sig = np.linspace(1.0, 3.0, B)
psfs = np.stack([synth.gaussian_psf(15, s) for s in sig])
# 16 seeded ground-truth images, each blurred with the PSF of the plane it lands on
y = np.empty((B, 1, 256, 256), np.float32)
for b in range(B):
    y[b] = synth.make_batch(1, 256, 256, psfs[b], g0=b % 16)[0]
y = torch.from_numpy(y).to(dev)
h = torch.from_numpy(psfs).to(dev).reshape(B, 1, 15, 15)
lam = torch.full((1,), LAM, device=dev)
rho = torch.full((1,), RHO, device=dev)
out = torch.empty_like(y)


def grouped():
    admm_deconv.tvd_fft_grouped(y, lam, rho, h, False, K, out=out)


def loop():
    for b in range(B):
        admm_deconv.tvd_fft(y[b:b + 1], lam, rho, h[b, 0], False, K, out=out[b:b + 1])


def ceiling():
    admm_deconv.tvd_fft(y, lam, rho, h[B // 2, 0], False, K, out=out)


def train():
    x, rec = admm_deconv.tvd_fft_grouped_record(y, lam, rho, h, False, K)
    return admm_deconv.tvd_fft_grouped_backward_recorded(rec, x, x - y)[1]


def train_loop():
    for b in range(B):
        x, rec = admm_deconv.tvd_fft_record(y[b:b + 1], lam, rho, h[b, 0], False, K)
        admm_deconv.tvd_fft_backward_recorded(rec, x, x - y[b:b + 1])


def train_ceiling():
    x, rec = admm_deconv.tvd_fft_record(y, lam, rho, h[B // 2, 0], False, K)
    return admm_deconv.tvd_fft_backward_recorded(rec, x, x - y)[1]


def profiled(fn):
    """Per-class milliseconds of one call under the library profiler (it synchronises: not the timed runs)."""
    from admm_deconv import _lib
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        return {name: round(_lib.profile_get(c)[0], 3) for c, name in _lib.KERNEL_CLASSES.items() if _lib.profile_get(c)[1]}
    finally:
        _lib.profile_enable(False)


for mode in args.modes.split(","):
    fn = {"grouped": grouped, "loop": loop, "ceiling": ceiling, "train": train, "train_loop": train_loop,
          "train_ceiling": train_ceiling}[mode]
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b_.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b_))
    med = statistics.median(ms)
    line = {"tool": "bench_grouped", "tag": args.tag, "mode": mode, "batch": B, "maxit": K, "groups": B,
            "steps": args.steps, "warmup": args.warmup, "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
            "ms_max": round(max(ms), 4), "img_per_s": round(B / med * 1e3, 1)}
    if mode.startswith("train"):
        hb = fn()   # (train_loop returns nothing: its gradients are per call)
        line["checksum"] = float(hb.double().sum().item()) if hb is not None else None
    else:
        line["checksum"] = float(out.double().sum().item())
    if args.profile:
        line["profile_ms"] = profiled(fn)
    print(json.dumps(line), flush=True)
