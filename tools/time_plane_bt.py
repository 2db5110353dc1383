"""Time the per-plane isotropic solve (isotropic="plane", ADMM_ISO_PLANE) against the other two proxes.

  python tools/time_plane_bt.py [c2] [c4] [vga]        (default: all three batches)

Batches: c2 (512 x 256^2, 15x15 PSF, K = 25), c4 (256 x 512^2 x 3, K = 50), vga (64 x 480x640, K = 25).  For each, the
median of WINDOWS windows of REPS calls between device events (after warm-up) of
  plane        isotropic="plane" (the 2-pass kernels at the power-of-two shapes, the runtime-length ones at 480x640)
  aniso_same   the anisotropic solve forced onto the same path (FUSED 0, SMOOTH 0, RESIDENT 0, MALL_STREAMS 1)
  batch        the batch-coupled isotropic solve on its default path
  batch_same   the batch-coupled isotropic solve forced to the 2-pass / runtime-length kernels
with the library profiler's per-class times of one call of each, and at c2 the record + sweep step (K = 25) of the three
proxes.  Byte model: the block-threshold line pass moves the anisotropic pass's 36 B/px plus one halo line of channel 1
per block (+4 / T B/px, T = 8) and costs one sqrt and one rcp per pixel, so plane / aniso_same should sit at about
1.01-1.02.  One condition holds by construction and is asserted: plane is no slower than batch_same (fewer bytes, half
the launches, no reduction).  Writes $OUT_DIR/plane_bt_bench.json (default bench_out/; profiles/plane_bt_bench.json
was written that way)."""
import contextlib
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "admm-deconv_amd"))

WINDOWS, REPS, WARM = 5, 3, 2
BATCHES = {
    "c2": dict(B=512, P=1, N=256, M=256, K=25),
    "c4": dict(B=256, P=3, N=512, M=512, K=50),
    "vga": dict(B=64, P=1, N=480, M=640, K=25),
}
PSF = (15, 2.5)
SAME_PATH = {"FUSED": 0, "SMOOTH": 0, "RESIDENT": 0, "MALL_STREAMS": 1}


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


def profile_classes(fn):
    import torch
    from admm_deconv import _lib
    _lib.profile_reset()
    _lib.profile_enable(True)
    fn()
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    out = {}
    for cls, name in _lib.KERNEL_CLASSES.items():
        ms, n = _lib.profile_get(cls)
        if n:
            out[name] = {"ms": round(ms, 4), "launches": n}
    _lib.profile_reset()
    return out


@contextlib.contextmanager
def options(opts):
    from admm_deconv import _lib
    with contextlib.ExitStack() as st:
        for k, v in opts.items():
            st.enter_context(_lib.option(k, v))
        yield


def run_batch(name, cfg):
    import torch
    import admm_deconv
    from admm_deconv import _lib, ops, synth
    dev = torch.device("cuda", 0)
    B, P, N, M, K = (cfg[k] for k in ("B", "P", "N", "M", "K"))
    psf = synth.gaussian_psf(*PSF)
    y = torch.from_numpy(synth.make_batch(8, M, N, psf, P=P)).to(dev).repeat(B // 8, 1, 1, 1).contiguous()
    h = torch.from_numpy(psf).to(dev)
    one = lambda v: torch.tensor([v], dtype=torch.float32, device=dev)   # noqa: E731
    lam, rho = one(synth.LAMBDA), one(synth.RHO)
    variants = {"plane": ("plane", {}), "aniso_same": (False, SAME_PATH), "batch": (True, {}), "batch_same": (True, SAME_PATH)}
    res = {"config": dict(cfg, psf=list(PSF), windows=WINDOWS, reps=REPS)}
    for vname, (iso, opts) in variants.items():
        with options(opts):
            fn = lambda: admm_deconv.tvd_fft(y, lam, rho, h, iso, K)   # noqa: E731
            r = timed(fn)
            r["path"] = _lib.query_paths(M, N, iso, PSF[0], planes=B * P)[0]
            r["classes"] = profile_classes(fn)
        res[vname] = r
        print(name, vname, json.dumps({k: r[k] for k in ("ms", "spread", "path")}), flush=True)
    res["ratio_plane_over_aniso_same"] = round(res["plane"]["ms"] / res["aniso_same"]["ms"], 4)
    res["ratio_plane_over_batch"] = round(res["plane"]["ms"] / res["batch"]["ms"], 4)
    res["plane_no_slower_than_batch_same"] = res["plane"]["ms"] <= res["batch_same"]["ms"]
    if name == "c2":   # the training step: record + reverse sweep (every gradient, h_bar included)
        xbar = torch.randn_like(y)
        step = {}
        for vname, (iso, opts) in variants.items():
            with options(opts):
                def fn():
                    x, rec = ops.tvd_fft_record(y, lam, rho, h, iso, K)
                    return ops.tvd_fft_backward_recorded(rec, x, xbar)
                r = timed(fn)
                r["paths"] = list(_lib.query_paths(M, N, iso, PSF[0], mode=_lib.MODE_RECORD, flags=_lib.REC_HBAR,
                                                   want_hbar=True, want_rho=True, planes=B * P))
                r["classes"] = profile_classes(fn)
            step[vname] = r
            print(name, "record+sweep", vname, json.dumps({k: r[k] for k in ("ms", "spread", "paths")}), flush=True)
        res["record_sweep"] = step
    del y
    torch.cuda.empty_cache()
    return res


def main():
    names = [a for a in sys.argv[1:] if a in BATCHES] or list(BATCHES)
    out_dir = os.environ.get("OUT_DIR", "bench_out")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "plane_bt_bench.json")
    res = json.load(open(path)) if os.path.exists(path) and len(names) < len(BATCHES) else {}
    for n in names:
        res[n] = run_batch(n, BATCHES[n])
        json.dump(res, open(path, "w"), indent=1)
    print(json.dumps({n: {k: res[n][k] for k in ("ratio_plane_over_aniso_same", "ratio_plane_over_batch",
                                                 "plane_no_slower_than_batch_same")} for n in names}))
    slow = [n for n in names if not res[n]["plane_no_slower_than_batch_same"]]
    assert not slow, f"isotropic per plane slower than the batch-coupled solve on the same kernels at {slow}"


if __name__ == "__main__":
    main()
