"""The fused 256 x 256 kernel's LDS hand-offs (csrc/plane_kernel.hip): the column buffer, the staging slots of the
row phase and the two boundary-line buffers (x of each wave's last line, w1 of each wave's first line) carry every
value between the lanes of a plane.  Three planes (an odd count) with and without a 3 x 3 PSF, at K = 1 (no row
phase), K = 2 (one row phase: zero-size s load, dropped s store) and K = 3 (the first real s round trip).

Plane 2 is the band image: the first and last line of every 32-line band (the lines of one wave) sit a step above /
below their neighbours, so the difference across every wave boundary is 0.6 where a smooth image has ~1e-2 -- a
wrong boundary line moves the lines around it by ~1e-2 and more, not by 1e-6.

Bounds: fused against 2-pass per-plane rel-L2 < 2e-5 (tests/test_gpu_default_rule.py: two fp32 paths, each within
1e-5 of the oracle); against the fp64 oracle tests/parity.py's rule; everything else bitwise."""
import numpy as np
import pytest
import torch

import admm_deconv
from admm_deconv import _lib, synth
from parity import MAXABS_TOL, assert_parity_fp32ref, oracle_solve

pytestmark = pytest.mark.gpu

M = 256
# tau = lam / rho = 0.0195: with noise of sigma 0.05 the prox is live from the first row phase on
LAM, RHO, SIGMA = 0.0041, 0.21, 0.05
CASES = [(psf, K) for psf in (False, True) for K in (1, 2, 3)]
IDS = [f"{'psf3' if p else 'nopsf'}-K{k}" for p, k in CASES]
EDGE_ROWS = np.array([r for r in range(M) if r % 32 in (0, 31)])


def band_image():
    """Lines r = 0 (mod 32) at 0.8, r = 31 (mod 32) at 0.2, the others at 0.5, with a step along the lines as well
    (so that both difference directions are live at every boundary pixel) and the noise of the other planes."""
    img = np.full((M, M), 0.5, np.float32)
    img[np.arange(M) % 32 == 0] = 0.8
    img[np.arange(M) % 32 == 31] = 0.2
    img[:, M // 2:] += 0.1
    return img + synth.noise(977, M * M, SIGMA).reshape(M, M).astype(np.float32)


_cache = {}


def _inputs(psf):
    if ("in", psf) not in _cache:
        h = synth.gaussian_psf(3, 0.8) if psf else None
        y = synth.make_batch(3, M, M, h, g0=40, sigma=SIGMA)
        y[2, 0] = band_image()
        _cache[("in", psf)] = (y, h)
    return _cache[("in", psf)]


def _run(dev, psf, K):
    """Every solve of one case, once: the fused kernel twice, the 2-pass path, both recording forwards, the oracle."""
    if (psf, K) in _cache:
        return _cache[(psf, K)]
    y, h = _inputs(psf)
    kh = 3 if psf else 0
    assert _lib.get_option("MIN_PLANES") == 0
    assert _lib.query_paths(M, M, False, kh, planes=3)[0] == "fused"
    yt = torch.from_numpy(y).to(dev)
    ht = torch.from_numpy(h).to(dev) if psf else None
    r = {}
    for name in ("fused", "again"):
        r[name] = admm_deconv.tvd_fft(yt, LAM, RHO, ht, False, K).cpu().numpy()
    with _lib.option("FUSED", 0):
        assert _lib.query_paths(M, M, False, kh, planes=3)[0] == "2pass"
        r["2pass"] = admm_deconv.tvd_fft(yt, LAM, RHO, ht, False, K).cpu().numpy()
    # need_h=False: a recording for h_bar keeps the dim-2 spectra, which the fused kernel never forms (2-pass forward)
    for name, need_rho in (("rec_full", True), ("rec_mask", False)):
        flags = 0 if need_rho else _lib.REC_MASKS
        assert _lib.query_paths(M, M, False, kh, mode=_lib.MODE_RECORD, flags=flags, planes=3)[0] == "fused"
        x, rec = admm_deconv.tvd_fft_record(yt, torch.tensor([LAM], device=dev), RHO, ht, False, K, need_h=False,
                                            need_rho=need_rho)
        assert rec.flags == flags
        r[name] = x.cpu().numpy()
    torch.cuda.synchronize()
    r["ref"] = oracle_solve(y, LAM, RHO, h, False, K, "spectral", linear_only=(K == 1), what=f"psf={psf} K={K}")
    _cache[(psf, K)] = r
    return r


@pytest.mark.parametrize("psf,K", CASES, ids=IDS)
def test_fused_vs_2pass(dev, psf, K):
    r = _run(dev, psf, K)
    a = r["fused"].reshape(3, -1).astype(np.float64)
    b = r["2pass"].reshape(3, -1).astype(np.float64)
    rel = np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)
    print(f"fused vs 2-pass per-plane rel-L2 {rel}")
    assert rel.max() < 2e-5, rel


@pytest.mark.parametrize("psf,K", CASES, ids=IDS)
def test_fused_vs_oracle(dev, psf, K):
    r = _run(dev, psf, K)
    y, h = _inputs(psf)
    w, m, e32 = assert_parity_fp32ref(r["fused"], r["ref"], y, LAM, RHO, h, False, K, what=f"fused psf={psf} K={K}")
    print(f"fused vs fp64 oracle: rel-L2 {w:.2e}, max-abs {m:.2e}, fp32 reference {e32}")


@pytest.mark.parametrize("psf,K", CASES, ids=IDS)
def test_recording_forwards_give_the_plain_x_bitwise(dev, psf, K):
    r = _run(dev, psf, K)
    assert np.array_equal(r["rec_full"], r["fused"]), "full-trajectory recording"
    assert np.array_equal(r["rec_mask"], r["fused"]), "mask-bit recording"


@pytest.mark.parametrize("psf,K", CASES, ids=IDS)
def test_two_runs_bitwise_equal(dev, psf, K):
    r = _run(dev, psf, K)
    assert np.array_equal(r["fused"], r["again"])


@pytest.mark.parametrize("psf,K", CASES, ids=IDS)
def test_band_image_boundary_lines(dev, psf, K):
    """The lines on either side of every wave boundary of the band image, against the fp64 oracle at the parity
    rule's max-abs guard (2e-4 of max|ref|; a wrong boundary line is off by ~1e-2 or more)."""
    r = _run(dev, psf, K)
    got, ref = r["fused"][2, 0].astype(np.float64), np.asarray(r["ref"], np.float64)[2, 0]
    # the boundaries matter: across them the solution steps by far more than the bound
    jump = np.abs(ref[32::32] - ref[31:-1:32]).mean()
    assert jump > 0.1, jump
    err = np.abs(got[EDGE_ROWS] - ref[EDGE_ROWS]).max() / np.abs(ref).max()
    print(f"band image: boundary-line max-abs {err:.2e} of max|ref|, mean step across a boundary {jump:.3f}")
    assert err <= MAXABS_TOL, err
