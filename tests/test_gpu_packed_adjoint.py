"""The fused reverse sweep (plane256_adj_kernel) with the packed-FP32 register transforms against the scalar build.

A scalar twin of the whole sweep would be a second copy of the library, so the reference here is a recording:
tests/golden/packed_adjoint_scalar.json holds what the library built with the scalar forms (the commit before
csrc/fft_pk.hpp) returned for this case -- 2 planes of 256 x 256, 15 x 15 PSF, K = 3, the full-trajectory variant
(rho_bar wanted) and the mask variant (not wanted), h_bar not wanted (with it the library takes the 2-pass sweep):
SHA-256 of the bytes of x and y_bar, and the bits of lambda_bar and rho_bar.  The packed forms are the scalar
operations with the same roundings, so every bit must agree.
"""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packed_adjoint_scalar.json")
LAM, RHO, K = 0.0041, 0.021, 3
VARIANTS = {"full": True, "mask": False}   # need_rho


def case():
    from admm_deconv import synth
    psf = synth.gaussian_psf(15, 2.5)
    y = synth.make_batch(2, 256, 256, psf).astype(np.float32)
    x_bar = np.random.default_rng(23).standard_normal(y.shape).astype(np.float32)
    return y, x_bar, np.asarray(psf, dtype=np.float32)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run(dev, need_rho):
    """{name: value} of one reverse sweep, in the form the recording keeps; the per-plane kernels forced."""
    import torch
    import admm_deconv
    from admm_deconv import _lib
    y, x_bar, psf = case()
    with _lib.option("MIN_PLANES", 0):
        fwd, bwd = _lib.query_paths(256, 256, False, 15, _lib.MODE_BACKWARD, 0, False, need_rho, planes=2)
        x, y_bar, h_bar, lam_bar, rho_bar = admm_deconv.ops.tvd_fft_backward(
            torch.from_numpy(y).to(dev), torch.from_numpy(x_bar).to(dev), LAM, RHO, torch.from_numpy(psf).to(dev),
            False, K, need_h=False, need_rho=need_rho)
        torch.cuda.synchronize()
    assert h_bar is None
    out = {"paths": [fwd, bwd], "x": sha(x.cpu().numpy()), "y_bar": sha(y_bar.cpu().numpy()),
           "lam_bar": int(lam_bar.cpu().numpy().astype(np.float32).view(np.uint32))}
    if need_rho:
        out["rho_bar"] = int(rho_bar.cpu().numpy().astype(np.float32).view(np.uint32))
    return out


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_fused_adjoint_bitwise_vs_scalar_recording(dev, variant):
    want = json.load(open(GOLDEN))[variant]
    got = run(dev, VARIANTS[variant])
    assert "plane" in got["paths"][1] or "fused" in got["paths"][1], got["paths"]
    assert got["paths"] == want["paths"]
    for key in want:
        assert got[key] == want[key], f"{variant}: {key} differs from the scalar build's recording"
