"""GPU: the grouped solve (admm_deconv.tvd_fft_grouped -> admm_tvd_forward_grouped_dev_f32) -- a PSF, lambda and rho per
image or channel in one call -- against the fp64 grouped oracle (tests/grouped_oracle.py), and bitwise against the
single-PSF solve of each plane through the same kernels."""
import numpy as np
import pytest
import torch

import admm_deconv
import oracle_np
from admm_deconv import _lib, synth
from grouped_oracle import group_of, tvd_fft_grouped as oracle_grouped
from parity import assert_parity, assert_parity_fp32ref, assert_prox_active

pytestmark = pytest.mark.gpu


def rand_psf(rng, kh, kw):
    h = rng.random((kw, kh)).astype(np.float32)
    return (h / h.sum()).astype(np.float32)


def lopsided_psf(rng):
    """9 x 9, zero-free, its weight in a 4 x 9 block (kh x kw = 9 x 9 with 4 x 9 content); its transpose is the
    9 x 4 content of the other group."""
    h = rng.random((9, 9)).astype(np.float32) + np.float32(1e-3)
    h[:, 4:] *= np.float32(0.05)
    return (h / h.sum()).astype(np.float32)


def make_psfs(spec, G, rng):
    """The groups' PSFs (kw, kh), drawn in group order."""
    if spec is None:
        return None
    if spec[0] == "rand":
        return [rand_psf(rng, spec[1], spec[2]) for _ in range(G)]
    if spec[0] == "transposed":
        h = lopsided_psf(rng)
        return [h, np.ascontiguousarray(h.T)]
    if spec[0] == "mixed15":
        return [synth.gaussian_psf(15, 2.5), synth.gaussian_psf(15, 1.0), rand_psf(rng, 15, 15)][:G]
    raise ValueError(spec)


def make_planes(B, P, N, M, hs, gb, gp):
    y = np.empty((B, P, N, M), np.float32)
    for b in range(B):
        for p in range(P):
            h = None if hs is None else hs[group_of(b, p, gb, gp)]
            y[b, p] = synth.make_batch(1, M, N, h, P=1, g0=7 + b * P + p)[0, 0]
    return y


def group_params(lam, rho, nparam):
    g = np.arange(nparam, dtype=np.float32)
    return (np.float32(lam) * (1 + np.float32(0.25) * g)).astype(np.float32), \
        (np.float32(rho) * (1 + np.float32(0.5) * g)).astype(np.float32)


def make_case(B, P, N, M, gb, gp, psf, lam, rho, K, iso, nparam):
    rng = np.random.default_rng(B * 1000 + N + M + K)
    hs = make_psfs(psf, gb * gp, rng)
    y = make_planes(B, P, N, M, hs, gb, gp)
    lams, rhos = group_params(lam, rho, nparam)
    return y, hs, lams, rhos


def run_grouped(dev, y, hs, gb, gp, lams, rhos, iso, K):
    """The grouped call on device copies of the inputs; every call also checks that the DEVICE y is unmodified."""
    h = None if hs is None else torch.from_numpy(np.stack(hs).reshape(gb, gp, *hs[0].shape)).to(dev)
    yd = torch.from_numpy(y).to(dev)
    x = admm_deconv.tvd_fft_grouped(yd, torch.from_numpy(lams).to(dev), torch.from_numpy(rhos).to(dev), h, iso, K)
    torch.cuda.synchronize()
    assert not x.requires_grad
    assert x.data_ptr() != yd.data_ptr()
    assert torch.equal(yd.cpu(), torch.from_numpy(y)), "the grouped call modified its input y on the device"
    return x.cpu().numpy()


def run_single(dev, yp, lam, rho, h, iso, K):
    ht = None if h is None else torch.from_numpy(np.ascontiguousarray(h)).to(dev)
    x = admm_deconv.tvd_fft(torch.from_numpy(np.ascontiguousarray(yp)).to(dev), float(lam), float(rho), ht, iso, K)
    torch.cuda.synchronize()
    return x.cpu().numpy()


# (B, P, N, M, gb, gp, PSF, lambda, rho, K, isotropic, nparam, path)
CASES = [
    (3, 2, 16, 8, 3, 1, ("rand", 3, 2), 0.05, 0.3, 5, False, 3, "2pass"),
    (2, 3, 16, 8, 2, 3, ("rand", 3, 2), 0.05, 0.3, 5, True, 1, "2pass_iso"),
    (2, 2, 64, 32, 1, 2, ("transposed",), 0.02, 0.1, 4, False, 2, "2pass"),
    (2, 3, 45, 63, 2, 3, ("rand", 10, 10), 0.02, 0.1, 6, False, 6, "runtime"),       # odd sides, even PSF
    (1, 3, 50, 33, 1, 3, ("rand", 4, 7), 0.02, 0.1, 7, True, 1, "runtime"),
    (2, 1, 30, 40, 2, 1, ("rand", 40, 30), 0.0002, 0.3, 9, False, 2, "runtime"),     # kh = M, kw = N
    (3, 2, 256, 256, 3, 1, ("mixed15",), 0.0041, 0.021, 5, False, 3, "fused"),       # (ADMM_OPT_MIN_PLANES 0)
    (2, 2, 16, 16, 2, 2, None, 0.05, 0.02, 6, False, 4, "2pass"),                    # no PSF, a pair per plane
]


def _cid(c):
    return f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-g{c[4]}x{c[5]}-K{c[9]}{'-iso' if c[10] else ''}"


@pytest.mark.parametrize("case", CASES, ids=[_cid(c) for c in CASES])
def test_grouped_parity_vs_oracle(dev, case):
    B, P, N, M, gb, gp, psf, lam, rho, K, iso, nparam, path = case
    y, hs, lams, rhos = make_case(B, P, N, M, gb, gp, psf, lam, rho, K, iso, nparam)
    kh = 0 if hs is None else hs[0].shape[1]
    assert _lib.query_grouped_path(M, N, iso, kh, B * P, gb * gp) == path
    st = {}
    ref = oracle_np.to_c(oracle_grouped(oracle_np.from_c(y.astype(np.float64)), lams, rhos,
                                        None if hs is None else [oracle_np.psf_from_c(h) for h in hs], gb, gp, iso, K,
                                        stats=st))
    frac = assert_prox_active(oracle_np.prox_active_fraction(st), str(case))
    got = run_grouped(dev, y, hs, gb, gp, lams, rhos, iso, K)
    if iso:
        w, m = assert_parity(got, ref, what=str(case))
        print(f"{_cid(case)}: prox live {frac:.3f}, rel-L2 {w:.2e}, max-abs {m:.2e}")
        return
    # anisotropic planes are independent.  Only a random PSF (ill-conditioned spectrum) may fall back to the fp32
    # reference solve's own error; a plane without a PSF or with a Gaussian one is held to 1e-5 / 2e-4 outright.
    random_psf = [False] * (gb * gp) if hs is None else \
        [psf[0] in ("rand", "transposed") or (psf[0] == "mixed15" and g == 2) for g in range(gb * gp)]
    for b in range(B):
        for p in range(P):
            g = group_of(b, p, gb, gp)
            gs = g if nparam > 1 else 0
            if not random_psf[g]:
                w, m = assert_parity(got[b:b + 1, p:p + 1], ref[b:b + 1, p:p + 1], what=f"{case} plane ({b}, {p})")
                print(f"{_cid(case)} ({b},{p}): prox live {frac:.3f}, rel-L2 {w:.2e}, max-abs {m:.2e}")
                continue
            w, m, e32 = assert_parity_fp32ref(got[b:b + 1, p:p + 1], ref[b:b + 1, p:p + 1], y[b:b + 1, p:p + 1], lams[gs],
                                              rhos[gs], None if hs is None else hs[g], False, K,
                                              what=f"{case} plane ({b}, {p})")
            print(f"{_cid(case)} ({b},{p}): prox live {frac:.3f}, rel-L2 {w:.2e}, max-abs {m:.2e}, fp32 ref {e32}")


BITWISE = [
    # (B, P, N, M, gb, gp, PSF, K)
    (3, 2, 256, 256, 3, 2, ("rand", 15, 15), 4),     # the fused kernel, 6 planes
    (2, 3, 64, 32, 2, 3, ("rand", 4, 9), 4),         # 2-pass
    (2, 3, 45, 63, 2, 3, ("rand", 10, 10), 4),       # runtime-length
    (2, 3, 64, 32, 2, 1, None, 4),                   # no PSF, a pair per image
]


@pytest.mark.parametrize("case", BITWISE, ids=[f"{c[3]}x{c[2]}-g{c[4]}x{c[5]}" for c in BITWISE])
def test_each_plane_is_bitwise_its_single_solve(dev, case):
    B, P, N, M, gb, gp, psf, K = case
    G = gb * gp
    y, hs, lams, rhos = make_case(B, P, N, M, gb, gp, psf, 0.0041, 0.021, K, False, G)
    with _lib.option("SMOOTH", 0), _lib.option("RESIDENT", 0):
        got = run_grouped(dev, y, hs, gb, gp, lams, rhos, False, K)    # (checks the device y, see run_grouped)
        again = run_grouped(dev, y, hs, gb, gp, lams, rhos, False, K)
        assert np.array_equal(got, again), "two identical calls differ"
        for b in range(B):
            for p in range(P):
                g = group_of(b, p, gb, gp)
                one = run_single(dev, y[b:b + 1, p:p + 1], lams[g], rhos[g], None if hs is None else hs[g], False, K)
                assert np.array_equal(got[b, p], one[0, 0]), f"plane ({b}, {p}) differs from its single-PSF solve"
    assert np.abs(got[0, 0] - got[1, 0]).max() > 0


@pytest.mark.parametrize("iso", [False, True])
@pytest.mark.parametrize("N,M", [(256, 256), (64, 32), (45, 63)])
def test_one_group_is_bitwise_the_batch_solve(dev, N, M, iso):
    B, P, K = 2, 3, 4
    y, hs, lams, rhos = make_case(B, P, N, M, 1, 1, ("rand", 5, 5), 0.0041, 0.021, K, iso, 1)
    # the single-PSF call of these shapes through the kernels a grouped call takes
    with _lib.option("SMOOTH", 0), _lib.option("RESIDENT", 0), _lib.option("FUSED", 0 if iso else 1):
        got = run_grouped(dev, y, hs, 1, 1, lams, rhos, iso, K)
        ref = run_single(dev, y, lams[0], rhos[0], hs[0], iso, K)
    assert np.array_equal(got, ref)


# y is const: one case per path with and without a PSF (without one the solve reads y where H^T y would be), both
# proxes, and two calls on the same device tensor
Y_CONST = [(256, 256, "fused"), (64, 32, "2pass"), (45, 63, "runtime")]


@pytest.mark.parametrize("iso", [False, True], ids=["aniso", "iso"])
@pytest.mark.parametrize("psf", [None, ("rand", 3, 3)], ids=["nopsf", "psf"])
@pytest.mark.parametrize("N,M,path", Y_CONST, ids=[c[2] for c in Y_CONST])
def test_device_input_is_never_modified(dev, N, M, path, psf, iso):
    B, P, K = 2, 2, 3
    nparam = 1 if iso else 4
    y, hs, lams, rhos = make_case(B, P, N, M, 2, 2, psf, 0.0041, 0.021, K, iso, nparam)
    want = {"fused": "2pass_iso", "2pass": "2pass_iso"}.get(path, path) if iso else path
    assert _lib.query_grouped_path(M, N, iso, 0 if hs is None else 3, B * P, 4) == want
    h = None if hs is None else torch.from_numpy(np.stack(hs).reshape(2, 2, 3, 3)).to(dev)
    yd = torch.from_numpy(y).to(dev)
    lt, rt = torch.from_numpy(lams).to(dev), torch.from_numpy(rhos).to(dev)
    x1 = admm_deconv.tvd_fft_grouped(yd, lt, rt, h, iso, K)
    torch.cuda.synchronize()
    assert torch.equal(yd.cpu(), torch.from_numpy(y)), "y modified on the device"
    x2 = admm_deconv.tvd_fft_grouped(yd, lt, rt, h, iso, K)
    torch.cuda.synchronize()
    assert torch.equal(yd.cpu(), torch.from_numpy(y)) and torch.equal(x1, x2)
    assert torch.isfinite(x1).all() and (x1 - yd).abs().max().item() > 0


@pytest.mark.min_planes_rule
def test_fused_path_at_the_default_plane_rule(dev):
    """96 planes of 256 x 256 with 96 PSFs: the default rule hands the batch to the fused kernel."""
    B, K = 96, 3
    assert _lib.get_option("MIN_PLANES") == -1
    assert _lib.query_grouped_path(256, 256, False, 5, B, B) == "fused"
    y, hs, lams, rhos = make_case(B, 1, 256, 256, B, 1, ("rand", 5, 5), 0.0041, 0.021, K, False, B)
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        got = run_grouped(dev, y, hs, B, 1, lams, rhos, False, K)
        assert _lib.profile_get(_lib.K_PLANE)[1] == 1 and _lib.profile_get(_lib.K_COLUMN)[1] == 0
    finally:
        _lib.profile_enable(False)
    with _lib.option("MIN_PLANES", 0):
        for b in (0, 47, 95):
            one = run_single(dev, y[b:b + 1], lams[b], rhos[b], hs[b], False, K)
            assert np.array_equal(got[b], one[0]), f"plane {b}"


def test_maxit_zero_gives_zeros(dev):
    y, hs, lams, rhos = make_case(2, 2, 64, 32, 2, 2, ("rand", 3, 3), 0.01, 0.1, 0, False, 4)
    x = admm_deconv.tvd_fft_grouped(torch.from_numpy(y).to(dev), torch.from_numpy(lams).to(dev),
                                    torch.from_numpy(rhos).to(dev), torch.from_numpy(np.stack(hs).reshape(2, 2, 3, 3)).to(dev),
                                    False, 0, out=torch.full((2, 2, 64, 32), 7.0, device=dev))
    torch.cuda.synchronize()
    assert torch.count_nonzero(x).item() == 0


def test_python_entry_argument_checks(dev):
    y = torch.zeros(2, 3, 16, 16, device=dev)
    h = torch.full((2, 3, 3, 3), 1.0 / 9, device=dev)
    with pytest.raises(NotImplementedError, match="adjoint"):
        admm_deconv.tvd_fft_grouped(y, 0.05, 0.3, h.clone().requires_grad_(True), False, 2)
    with pytest.raises(NotImplementedError, match="adjoint"):
        admm_deconv.tvd_fft_grouped(y, torch.tensor([0.05], device=dev, requires_grad=True), 0.3, h, False, 2)
    with torch.no_grad():   # no graph is asked for: the forward runs
        x = admm_deconv.tvd_fft_grouped(y, 0.05, 0.3, h.clone().requires_grad_(True), False, 2)
    assert not x.requires_grad
    for shape in ((3, 3, 3, 3), (2, 2, 3, 3), (6, 1, 3, 3)):
        with pytest.raises(ValueError, match="leading dims"):
            admm_deconv.tvd_fft_grouped(y, 0.05, 0.3, torch.zeros(*shape, device=dev), False, 2)
    with pytest.raises(ValueError):
        admm_deconv.tvd_fft_grouped(y, torch.ones(4, device=dev), 0.3, h, False, 2)    # neither 1 nor gb * gp values
    # no PSF: the groups follow the parameter count, which must name them without a tie
    ysq = torch.zeros(3, 3, 16, 16, device=dev)
    with pytest.raises(ValueError, match="ambiguous"):
        admm_deconv.tvd_fft_grouped(ysq, torch.full((3,), 0.05, device=dev), 0.3, None, False, 2)
    with pytest.raises(ValueError):
        admm_deconv.tvd_fft_grouped(y, torch.full((5,), 0.05, device=dev), 0.3, None, False, 2)
    assert admm_deconv.tvd_fft_grouped(y, torch.full((3,), 0.05, device=dev), 0.3, None, False, 2).shape == y.shape
    with pytest.raises(admm_deconv.AdmmError) as e:   # the isotropic prox takes one (lambda, rho) pair
        admm_deconv.tvd_fft_grouped(y, torch.full((6,), 0.05, device=dev), 0.3, h, True, 2)
    assert e.value.code == _lib.ADMM_E_UNSUPPORTED
