"""The packed-FP32 forms of the fused 256x256 kernels' register transforms (csrc/fft_pk.hpp, ADMM_PK_F32) against
the scalar forms, bit for bit.

libadmm_devtest.so is built with the fused kernels' flags (packed forms); libadmm_devtest_scalar.so is the same
source with the scalar forms.  Every packed operation is the scalar one with the same roundings per component
(signs ride on constants, adds and subtracts on an FMA with +-1), so nothing may differ but the payload of a NaN.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import PKG_DIR

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p


def _load(name):
    path = os.path.join(PKG_DIR, name)
    if not os.path.exists(path):
        pytest.fail(f"{name} not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(path)
    for fn in ("devtest_pair_forward", "devtest_pair_inverse", "devtest_pair_inverse_staged"):
        getattr(lib, fn).argtypes = [P, P, ctypes.c_int]
    lib.devtest_prims.argtypes = [P, P, P]
    lib.devtest_plane_tables.argtypes = [P, P, P]
    lib.devtest_plane_tables_psf.argtypes = [P] * 6
    plane = [P] * 6 + [ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_int, P]
    lib.devtest_plane_debug.argtypes = plane
    lib.devtest_plane_wg_times.argtypes = plane
    lib.devtest_plane_debug_psf.argtypes = [P] * 8 + [ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_int, P]
    return lib


@pytest.fixture(scope="module")
def libs():
    packed, scalar = _load("libadmm_devtest.so"), _load("libadmm_devtest_scalar.so")
    assert packed.devtest_packed() == 1, "libadmm_devtest.so was built without ADMM_PK_F32"
    assert scalar.devtest_packed() == 0, "libadmm_devtest_scalar.so was built with ADMM_PK_F32"
    return packed, scalar


def assert_same_bits(got, want, what):
    """Bit for bit, except that a NaN matches any NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    g, w = got.view(np.uint32).ravel(), want.view(np.uint32).ravel()
    gf, wf = got.view(np.float32).ravel(), want.view(np.float32).ravel()
    bad = (g != w) & ~(np.isnan(gf) & np.isnan(wf))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        pytest.fail(f"{what}: {int(bad.sum())} of {g.size} words differ; first at {i}: packed {gf[i]!r} "
                    f"(0x{int(g[i]):08x}) scalar {wf[i]!r} (0x{int(w[i]):08x})")


SPECIALS = np.array([0.0, -0.0, 1e-40, -3e-42, np.inf, -np.inf, np.nan, 1.0, -1.0, 3e38, -2e-38, 0.5],
                    dtype=np.float32)


def test_primitives_bitwise(dev, libs):
    """cadd / csub / cmul / cscale / cconj / rot, w16<E> and w256<E> (trivial, diagonal and general E, both
    directions) and the dft<2 / 4 / 8 / 16> butterflies on one block of 64 threads: lanes 0..23 random values of
    mixed magnitude, lanes 24..63 combinations of +-0, denormals, +-inf, NaN and extreme finite values."""
    import torch
    packed, scalar = libs
    rng = np.random.default_rng(11)
    a = (rng.standard_normal((16, 64, 2)) * 10.0 ** rng.integers(-18, 18, size=(16, 64, 2))).astype(np.float32)
    a[:, :8] = rng.standard_normal((16, 8, 2)).astype(np.float32)
    j, t, c = np.meshgrid(np.arange(16), np.arange(24, 64), np.arange(2), indexing="ij")
    a[:, 24:] = SPECIALS[(5 * j + 7 * t + 3 * c + (t // 12) * j * c) % len(SPECIALS)]
    a[:, 44:, 1] = rng.standard_normal((16, 20)).astype(np.float32)   # a special against an ordinary component
    outs = []
    nslots = packed.devtest_prims_slots()
    assert nslots == scalar.devtest_prims_slots()
    for lib in libs:
        inp = torch.from_numpy(a).to(dev)
        out = torch.full((nslots, 64, 2), 7.0, device=dev)
        n = torch.zeros(1, dtype=torch.int32, device=dev)
        assert lib.devtest_prims(inp.data_ptr(), out.data_ptr(), n.data_ptr()) == 0
        assert int(n.item()) == nslots
        outs.append(out.cpu().numpy())
    assert_same_bits(outs[0], outs[1], "primitives")
    assert np.isfinite(outs[1][:, :8]).all()


@pytest.fixture(scope="module")
def line_data():
    rng = np.random.default_rng(5)
    rows = 256   # one block of 512 threads: every lane-pair role, registers 0 and 32 included
    x = rng.standard_normal((rows, 256)).astype(np.float32)
    spec = (rng.standard_normal((rows, 128, 2))).astype(np.float32)
    return rows, x, spec


@pytest.mark.parametrize("which", ["forward", "inverse", "inverse_staged"])
def test_line_transforms_bitwise(dev, libs, line_data, which):
    import torch
    rows, x, spec = line_data
    outs = []
    for lib in libs:
        if which == "forward":
            src = torch.from_numpy(x).to(dev)
            dst = torch.zeros((rows, 128, 2), device=dev)
        else:
            src = torch.from_numpy(spec).to(dev)
            dst = torch.zeros((rows, 256), device=dev)
        assert getattr(lib, f"devtest_pair_{which}")(src.data_ptr(), dst.data_ptr(), rows) == 0
        outs.append(dst.cpu().numpy())
    assert np.abs(outs[1]).max() > 1.0
    assert_same_bits(outs[0], outs[1], f"line {which}")


def _tables(M, N, rho, psf):
    k = np.arange(M // 2 + 1)[None, :]
    kj = np.arange(N)[:, None]
    lap = 4 * np.sin(np.pi * kj / N) ** 2 + 4 * np.sin(np.pi * k / M) ** 2
    if psf is None:
        return (1.0 / (1.0 + rho * lap) / (M * N)).astype(np.float32), None
    pad = np.zeros((N, M))
    kh, kw = psf.shape
    pad[:kh, :kw] = psf
    pad = np.roll(pad, (-(kh // 2), -(kw // 2)), axis=(0, 1))
    H = np.fft.fft2(pad)[:, :M // 2 + 1]
    Ct = (1.0 / (np.abs(H) ** 2 + rho * lap) / (M * N)).astype(np.float32)
    Gt = (np.conj(H) / (M * N)).astype(np.complex64)
    return Ct, Gt


@pytest.mark.parametrize("variant", ["plain", "psf", "staged"])
def test_fused_forward_bitwise(dev, libs, variant):
    """plane256_kernel at 2 planes, K = 3 (the zero-s first iteration, a middle one that reads and stores s, the last
    one that stores none): x, the s and H^T y workspaces and (plain, psf) every per-phase dump.  `staged` is the
    product kernel's own path (the staged line inverse) without the dumps."""
    import torch
    from admm_deconv import synth
    M = N = 256
    lam, rho, K, B = 0.0041, 0.021, 3, 2
    psf = synth.gaussian_psf(15, 2.5) if variant == "psf" else None
    Ct, Gt = _tables(M, N, rho, None if psf is None else np.asarray(psf, dtype=np.float64))
    y = synth.make_batch(B, M, N, psf).astype(np.float32)
    res = []
    for lib in libs:
        Ctd = torch.from_numpy(Ct.ravel()).to(dev)
        Cf = torch.zeros(2 * 32 * 512, device=dev)
        C0b = torch.zeros(256, device=dev)
        yt = torch.from_numpy(y).to(dev).contiguous()
        x = torch.zeros_like(yt)
        hln = torch.zeros(B * (64 * 512 + 128) * 2, device=dev)
        sln = torch.zeros(B * 64 * 512 * 4, device=dev)
        dbg = torch.zeros((4 * K + 1) * 64 * 512 * 2, device=dev)
        if variant == "psf":
            Gtd = torch.from_numpy(Gt.view(np.float32).ravel()).to(dev)
            Gf = torch.zeros(2 * 32 * 512 * 2, device=dev)
            G0b = torch.zeros(256 * 2, device=dev)
            assert lib.devtest_plane_tables_psf(Ctd.data_ptr(), Gtd.data_ptr(), Cf.data_ptr(), C0b.data_ptr(),
                                                Gf.data_ptr(), G0b.data_ptr()) == 0
            assert lib.devtest_plane_debug_psf(yt.data_ptr(), x.data_ptr(), Cf.data_ptr(), C0b.data_ptr(), Gf.data_ptr(),
                                               G0b.data_ptr(), hln.data_ptr(), sln.data_ptr(), lam / rho, rho, K, B,
                                               dbg.data_ptr()) == 0
        else:
            assert lib.devtest_plane_tables(Ctd.data_ptr(), Cf.data_ptr(), C0b.data_ptr()) == 0
            fn = lib.devtest_plane_debug if variant == "plain" else lib.devtest_plane_wg_times
            assert fn(yt.data_ptr(), x.data_ptr(), Cf.data_ptr(), C0b.data_ptr(), hln.data_ptr(), sln.data_ptr(),
                      lam / rho, rho, K, B, dbg.data_ptr()) == 0
        if variant == "staged":
            dbg.zero_()   # clock stamps
        res.append([a.cpu().numpy() for a in (x, sln, hln, dbg)])
    want = res[1]
    assert np.isfinite(want[0]).all() and np.abs(want[0]).max() > 0.1 and np.abs(want[1]).max() > 0
    for got, ref, what in zip(res[0], want, ("x", "s workspace", "H^T y workspace", "phase dumps")):
        assert_same_bits(got, ref, f"{variant}: {what}")
