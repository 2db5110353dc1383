"""GPU: the grouped adjoint (admm_deconv.tvd_fft_grouped_backward / _record / _backward_recorded / _grad ->
admm_tvd_backward_grouped_*): gradients per PSF / (lambda, rho) group from one recorded forward and one reverse sweep.
  a. against autograd of the fp64 grouped oracle (tests/grouped_oracle_torch.py), with test_gpu_backward.py's bounds:
     y_bar 1 % trimmed rel-L2 <= 1e-4 and full <= 5e-3, each lambda_bar_g / rho_bar_g relative <= 1e-3, each h_bar_g
     relative L2 <= 1e-3 -- each relaxed to twice the error of an fp32 autograd of the same oracle where that is larger
     (that file's rule for ST mask flips);
  b. anisotropic, every plane against its own single-PSF adjoint through the same kernels: x and y_bar bitwise, the
     scalars and h_bar (the same fp64 partial rows summed in another order, rounded to fp32 once) within 2 fp32 ulps;
  c. consistency (record + replay = the combined call, determinism, dropped outputs, G = 1, refusals);
  d. autograd through tvd_fft_grouped_grad;
  e. the launches per profiler class of the 2-pass, runtime-length and fused-trajectory sequences equal
     tests/launch_counts.py GROUPED_COUNTS exactly."""
import functools

import numpy as np
import pytest
import torch

import admm_deconv
from admm_deconv import _lib
from grouped_oracle_torch import group_of, tvd_fft_grouped_grads
from launch_counts import CLASSES, GROUPED_COUNTS
from parity import assert_parity, assert_prox_active
from test_gpu_backward import assert_grad, grad_errs, rel
from test_gpu_grouped import make_case

pytestmark = pytest.mark.gpu


def to_dev(dev, y, hs, gb, gp, lams, rhos):
    h = None if hs is None else torch.from_numpy(np.stack(hs).reshape(gb, gp, *hs[0].shape)).to(dev)
    return torch.from_numpy(y).to(dev), torch.from_numpy(lams).to(dev), torch.from_numpy(rhos).to(dev), h


def seeded_xbar(shape, seed=23):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def run_combined(dev, y, hs, gb, gp, lams, rhos, iso, K, xbar, **kw):
    """tvd_fft_grouped_backward on device copies; checks that the DEVICE y is unmodified.  Returns device tensors."""
    yd, lt, rt, h = to_dev(dev, y, hs, gb, gp, lams, rhos)
    out = admm_deconv.tvd_fft_grouped_backward(yd, torch.from_numpy(xbar).to(dev), lt, rt, h, iso, K, **kw)
    torch.cuda.synchronize()
    assert torch.equal(yd.cpu(), torch.from_numpy(y)), "the grouped adjoint modified its input y on the device"
    return out


def run_recorded(dev, y, hs, gb, gp, lams, rhos, iso, K, xbar, need_h=True, **kw):
    yd, lt, rt, h = to_dev(dev, y, hs, gb, gp, lams, rhos)
    x, rec = admm_deconv.tvd_fft_grouped_record(yd, lt, rt, h, iso, K, need_h=need_h)
    out = admm_deconv.tvd_fft_grouped_backward_recorded(rec, x, torch.from_numpy(xbar).to(dev), **kw)
    torch.cuda.synchronize()
    assert torch.equal(yd.cpu(), torch.from_numpy(y)), "record / replay modified y on the device"
    return (x, *out), rec


def same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


def ulps(a, b):
    """Largest difference of two fp32 arrays in units of b's spacing."""
    a, b = np.asarray(a, np.float32).ravel(), np.asarray(b, np.float32).ravel()
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)))


# ---- a. against the grouped fp64 oracle ----------------------------------------------------------------------------
# (B, P, N, M, gb, gp, PSF, lambda, rho, K, isotropic, nparam, (forward, sweep) of a recording with h_bar)
CASES = [
    (3, 2, 16, 8, 3, 1, ("rand", 3, 2), 0.05, 0.3, 5, False, 3, ("2pass", "sweep_2pass")),          # per image
    (2, 3, 16, 8, 1, 3, ("rand", 3, 2), 0.05, 0.3, 5, False, 3, ("2pass", "sweep_2pass")),          # strided groups
    (3, 2, 16, 8, 3, 1, ("rand", 3, 2), 0.05, 0.3, 5, False, 1, ("2pass", "sweep_2pass")),          # one pair, 3 PSFs
    (2, 2, 64, 32, 1, 2, ("transposed",), 0.02, 0.1, 4, False, 2, ("2pass", "sweep_2pass")),
    (2, 2, 16, 16, 2, 2, None, 0.05, 0.02, 6, False, 4, ("2pass", "sweep_2pass")),                  # no PSF
    (2, 3, 45, 63, 2, 3, ("rand", 10, 10), 0.02, 0.1, 6, False, 6, ("runtime", "sweep_runtime")),   # even PSF
    (2, 2, 256, 256, 2, 1, ("mixed15",), 0.0041, 0.021, 3, False, 2, ("2pass", "sweep_2pass")),     # two Gaussians
    (2, 3, 16, 8, 2, 3, ("rand", 3, 2), 0.05, 0.3, 5, True, 1, ("2pass_iso", "sweep_2pass_iso")),
    (6, 3, 16, 16, 1, 3, ("rand", 3, 3), 0.05, 0.3, 5, True, 1, ("2pass_iso", "sweep_2pass_iso")),  # 2 ISO_ADJ_A groups
    (1, 3, 50, 33, 1, 3, ("rand", 4, 7), 0.02, 0.1, 7, True, 1, ("runtime", "sweep_runtime_iso")),
]


def _cid(c):
    return f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-g{c[4]}x{c[5]}-n{c[11]}-K{c[9]}{'-iso' if c[10] else ''}"


@functools.lru_cache(maxsize=None)
def reference(case):
    """Inputs and the oracle's gradients in fp64 and fp32, computed once per case and shared (never modified)."""
    B, P, N, M, gb, gp, psf, lam, rho, K, iso, nparam, _ = case
    y, hs, lams, rhos = make_case(B, P, N, M, gb, gp, psf, lam, rho, K, iso, nparam)
    xbar = seeded_xbar(y.shape)
    st = {}
    r64 = tvd_fft_grouped_grads(y.astype(np.float64), lams, rhos, None if hs is None else [h.astype(np.float64) for h in hs],
                                gb, gp, iso, K, xbar, stats=st)
    r32 = tvd_fft_grouped_grads(y, lams, rhos, hs, gb, gp, iso, K, xbar, dtype=torch.float32)
    return y, hs, lams, rhos, xbar, r64, r32, float(np.mean(st["prox_active"]))


def check_against_oracle(case, got, want_h):
    B, P, N, M, gb, gp, psf, lam, rho, K, iso, nparam, _ = case
    y, hs, lams, rhos, xbar, (x0, yb0, hb0, lb0, rb0), (_, yb32, hb32, lb32, rb32), frac = reference(case)
    assert_prox_active(frac, str(case))
    x, yb, hb, lb, rb = (None if t is None else t.cpu().numpy() for t in got)
    assert_parity(x, x0, what="x")
    t32, f32 = grad_errs(yb32, yb0)
    print(f"{_cid(case)}: prox live {frac:.3f}; y_bar errs {grad_errs(yb, yb0)} (fp32 autograd {t32:.1e}, {f32:.1e})")
    assert_grad(yb, yb0, "y_bar", tol=max(1e-4, 2 * t32), full_tol=max(5e-3, 2 * f32))
    assert lb.shape == rb.shape == (nparam,)
    for g in range(nparam):
        print(f"  lambda_bar[{g}] {rel(lb[g], lb0[g]):.1e} (fp32 {rel(lb32[g], lb0[g]):.1e}), "
              f"rho_bar[{g}] {rel(rb[g], rb0[g]):.1e} (fp32 {rel(rb32[g], rb0[g]):.1e})")
        assert rel(lb[g], lb0[g]) <= max(1e-3, 2 * rel(lb32[g], lb0[g])), f"lambda_bar[{g}]"
        assert rel(rb[g], rb0[g]) <= max(1e-3, 2 * rel(rb32[g], rb0[g])), f"rho_bar[{g}]"
    if not want_h:
        assert hb is None
        return
    assert hb.shape == (gb, gp, *hs[0].shape)
    hb = hb.reshape(gb * gp, *hs[0].shape)
    for g in range(gb * gp):
        e = np.linalg.norm(hb[g] - hb0[g]) / np.linalg.norm(hb0[g])
        e32 = np.linalg.norm(hb32[g] - hb0[g]) / np.linalg.norm(hb0[g])
        print(f"  h_bar[{g}] {e:.1e} (fp32 {e32:.1e})")
        assert e <= max(1e-3, 2 * e32), f"h_bar[{g}]"


@pytest.mark.parametrize("case", CASES, ids=[_cid(c) for c in CASES])
def test_grouped_adjoint_vs_oracle(dev, case):
    B, P, N, M, gb, gp, psf, lam, rho, K, iso, nparam, paths = case
    y, hs, lams, rhos, xbar = reference(case)[:5]
    kh = 0 if hs is None else hs[0].shape[1]
    assert _lib.query_grouped_paths(M, N, iso, kh, B * P, gb * gp, flags=_lib.REC_HBAR) == paths
    got = run_combined(dev, y, hs, gb, gp, lams, rhos, iso, K, xbar)
    check_against_oracle(case, got, hs is not None)


def test_fused_trajectory_vs_oracle(dev):
    """256 x 256 without h_bar above the plane-count rule (here ADMM_OPT_MIN_PLANES 0): the fused forward records s
    lane-native, the 2-pass sweep reads it with every plane's group scalars."""
    case = CASES[6]
    B, P, N, M, gb, gp, psf, lam, rho, K, iso, nparam, _ = case
    y, hs, lams, rhos, xbar = reference(case)[:5]
    with _lib.option("MIN_PLANES", 0):
        assert _lib.query_grouped_paths(M, N, iso, 15, B * P, gb * gp) == ("fused", "sweep_2pass")
        got = run_combined(dev, y, hs, gb, gp, lams, rhos, iso, K, xbar, need_h=False)
    check_against_oracle(case, got, False)


# ---- b. every plane against its own single-PSF adjoint through the same kernels -----------------------------------
BITWISE = [
    # (N, M, PSF, lambda, rho, K)
    (64, 32, ("rand", 4, 9), 0.0041, 0.021, 4),
    (45, 63, ("rand", 10, 10), 0.0041, 0.021, 4),
    (30, 40, ("rand", 40, 30), 0.0002, 0.3, 9),       # kh = M, kw = N
    (256, 256, ("rand", 15, 15), 0.0041, 0.021, 4),
    (64, 32, None, 0.0041, 0.021, 4),
]


@pytest.mark.parametrize("case", BITWISE, ids=[f"{c[1]}x{c[0]}{'' if c[2] else '-nopsf'}" for c in BITWISE])
def test_each_plane_matches_its_single_adjoint(dev, case):
    N, M, psf, lam, rho, K = case
    B, P = 2, 2
    y, hs, lams, rhos = make_case(B, P, N, M, B, P, psf, lam, rho, K, False, B * P)
    xbar = seeded_xbar(y.shape)
    with _lib.option("SMOOTH", 0), _lib.option("RESIDENT", 0), _lib.option("FUSED_ADJ", 0), _lib.option("MIN_PLANES", 0):
        variants = [True] if N != 256 or hs is None else [True, False]   # 256^2: the fused trajectory too (no h_bar)
        for need_h in variants:
            (x, yb, hb, lb, rb), _ = run_recorded(dev, y, hs, B, P, lams, rhos, False, K, xbar, need_h=need_h)
            yd, lt, rt, h = to_dev(dev, y, hs, B, P, lams, rhos)
            # (a 256 x 256 recording for h_bar runs the 2-pass forward: the plain call through the same kernels)
            with _lib.option("FUSED", 0 if N == 256 and need_h else 1):
                plain = admm_deconv.tvd_fft_grouped(yd, lt, rt, h, False, K)
            assert torch.equal(x, plain), "recorded x != tvd_fft_grouped"
            for b in range(B):
                for p in range(P):
                    g = group_of(b, p, B, P)
                    ht = None if hs is None else torch.from_numpy(hs[g]).to(dev)
                    x1, yb1, hb1, lb1, rb1 = admm_deconv.tvd_fft_backward(
                        yd[b:b + 1, p:p + 1].clone(), torch.from_numpy(xbar[b:b + 1, p:p + 1]).to(dev), float(lams[g]),
                        float(rhos[g]), ht, False, K, need_h=need_h)
                    torch.cuda.synchronize()
                    assert torch.equal(x[b, p], x1[0, 0]), f"x of plane ({b}, {p})"
                    assert torch.equal(yb[b, p], yb1[0, 0]), f"y_bar of plane ({b}, {p})"
                    ul, ur = ulps(lb[g].cpu(), lb1.cpu()), ulps(rb[g].cpu(), rb1.cpu())
                    print(f"{M}x{N} need_h={need_h} group {g}: lambda_bar {ul:.2f} ulp, rho_bar {ur:.2f} ulp")
                    assert ul <= 2 and ur <= 2
                    if need_h and hs is not None:
                        uh = ulps(hb[b, p].cpu(), hb1.cpu())
                        print(f"  h_bar {uh:.2f} ulp")
                        assert uh <= 2
                    else:
                        assert hb is None and hb1 is None


# ---- c. consistency ---------------------------------------------------------------------------------------------------
CONSIST = [CASES[1], CASES[5], CASES[7]]   # 2-pass with strided groups, runtime-length, 2-pass isotropic


@pytest.mark.parametrize("case", CONSIST, ids=[_cid(c) for c in CONSIST])
def test_record_replay_is_the_combined_call_and_outputs_can_be_dropped(dev, case):
    B, P, N, M, gb, gp, psf, lam, rho, K, iso, nparam, _ = case
    y, hs, lams, rhos = make_case(B, P, N, M, gb, gp, psf, lam, rho, K, iso, nparam)
    xbar = seeded_xbar(y.shape)
    full = run_combined(dev, y, hs, gb, gp, lams, rhos, iso, K, xbar)
    again = run_combined(dev, y, hs, gb, gp, lams, rhos, iso, K, xbar)
    assert all(same(a, b) for a, b in zip(full, again)), "two identical calls differ"
    replay, rec = run_recorded(dev, y, hs, gb, gp, lams, rhos, iso, K, xbar)
    assert all(same(a, b) for a, b in zip(full, replay)), "record + replay differs from the combined call"
    with pytest.raises(RuntimeError, match="consumed"):
        admm_deconv.tvd_fft_grouped_backward_recorded(rec, replay[0], torch.from_numpy(xbar).to(dev))
    for need_y, need_rho in ((False, True), (True, False), (False, False)):
        part = run_combined(dev, y, hs, gb, gp, lams, rhos, iso, K, xbar, need_y=need_y, need_rho=need_rho)
        x, yb, hb, lb, rb = part
        assert (yb is None) == (not need_y) and (rb is None) == (not need_rho)
        assert same(x, full[0]) and same(hb, full[2]) and same(lb, full[3])
        assert yb is None or same(yb, full[1])
        assert rb is None or same(rb, full[4])


@pytest.mark.parametrize("iso", [False, True], ids=["aniso", "iso"])
@pytest.mark.parametrize("N,M", [(64, 32), (45, 63)])
def test_one_group_is_the_single_adjoint(dev, N, M, iso):
    B, P, K = 2, 3, 4
    y, hs, lams, rhos = make_case(B, P, N, M, 1, 1, ("rand", 5, 5), 0.0041, 0.021, K, iso, 1)
    xbar = seeded_xbar(y.shape)
    with _lib.option("SMOOTH", 0), _lib.option("RESIDENT", 0):
        x, yb, hb, lb, rb = run_combined(dev, y, hs, 1, 1, lams, rhos, iso, K, xbar)
        x1, yb1, hb1, lb1, rb1 = admm_deconv.tvd_fft_backward(torch.from_numpy(y).to(dev), torch.from_numpy(xbar).to(dev),
                                                              float(lams[0]), float(rhos[0]), torch.from_numpy(hs[0]).to(dev),
                                                              iso, K)
        torch.cuda.synchronize()
    assert torch.equal(x, x1) and torch.equal(yb, yb1)
    assert ulps(lb.cpu(), lb1.cpu()) <= 2 and ulps(rb.cpu(), rb1.cpu()) <= 2 and ulps(hb[0, 0].cpu(), hb1.cpu()) <= 2


def test_maxit_zero_gives_zeros(dev):
    y, hs, lams, rhos = make_case(2, 2, 64, 32, 2, 2, ("rand", 3, 3), 0.01, 0.1, 0, False, 4)
    out = run_combined(dev, y, hs, 2, 2, lams, rhos, False, 0, seeded_xbar(y.shape))
    assert out[2].shape == (2, 2, 3, 3) and out[3].shape == out[4].shape == (4,)
    assert all(torch.count_nonzero(t).item() == 0 for t in out)


def test_replay_with_another_grouping_is_refused(dev):
    B, P, N, M, gb, gp, psf, lam, rho, K, iso, nparam, _ = CASES[0]
    y, hs, lams, rhos = make_case(B, P, N, M, gb, gp, psf, lam, rho, K, iso, nparam)
    yd, lt, rt, h = to_dev(dev, y, hs, gb, gp, lams, rhos)
    xb = torch.from_numpy(seeded_xbar(y.shape)).to(dev)
    x, rec = admm_deconv.tvd_fft_grouped_record(yd, lt, rt, h, iso, K)
    ws = rec.workspace
    for other in ({"nparam": 1}, {"gb": 1, "nparam": 1}):   # valid groupings of the same planes, not the recorded one
        good = {k: getattr(rec, k) for k in other}
        for k, v in other.items():
            setattr(rec, k, v)
        with pytest.raises(admm_deconv.AdmmError) as e:
            admm_deconv.tvd_fft_grouped_backward_recorded(rec, x, xb)
        assert e.value.code == _lib.ADMM_E_INVALID and "recording" in str(e.value)
        for k, v in good.items():
            setattr(rec, k, v)
        assert rec.workspace is ws   # the refused replay consumed nothing
    # a single-solve replay of the grouped recording's workspace is refused too
    single = admm_deconv.Recording()
    single.workspace, single.y4, single.hb, single.shape, single.dv = ws, yd, None, yd.shape, None
    single.lam, single.rho, single.iso, single.maxit, single.want_h, single.group = 0.05, 0.3, False, K, False, None
    single.dims, single.flags = (M, N, P, B, 0, 0), 0
    with pytest.raises(admm_deconv.AdmmError) as e:
        admm_deconv.tvd_fft_backward_recorded(single, x, xb)
    assert e.value.code == _lib.ADMM_E_INVALID
    rec.workspace = ws
    ref = admm_deconv.tvd_fft_grouped_backward(yd, xb, lt, rt, h, iso, K)
    out = admm_deconv.tvd_fft_grouped_backward_recorded(rec, x, xb)   # the recording is still whole
    torch.cuda.synchronize()
    assert all(same(a, b) for a, b in zip(ref[1:], out))


def test_replay_with_another_gp_is_refused(dev):
    B, P, N, M, gb, gp, psf, lam, rho, K, iso, nparam, _ = CASES[1]   # gb = 1, gp = P
    y, hs, lams, rhos = make_case(B, P, N, M, gb, gp, psf, lam, rho, K, iso, nparam)
    yd, lt, rt, h = to_dev(dev, y, hs, gb, gp, lams, rhos)
    x, rec = admm_deconv.tvd_fft_grouped_record(yd, lt, rt, h, iso, K)
    rec.gp, rec.nparam = 1, 1
    with pytest.raises(admm_deconv.AdmmError) as e:
        admm_deconv.tvd_fft_grouped_backward_recorded(rec, x, torch.ones_like(yd))
    assert e.value.code == _lib.ADMM_E_INVALID


# ---- launches per profiler class (tests/launch_counts.py GROUPED_COUNTS) -------------------------------------------
def grouped_launch_counts(dev, cid):
    """The launches per class of one grouped adjoint call: K = 4, B = 2, P = 3, a group per plane, 5 x 5 PSFs; cid =
    "MxN-prox-call-variant": call "replay" (record + replay, counted together) or "combined"; variant "h" (h_bar),
    "noh" (need_h=False) or "drop" (need_y=False, need_rho=False).  Also checks the path the call was planned on."""
    shape, prox, call, variant = cid.split("-")
    M, N = (int(v) for v in shape.split("x"))
    iso, B, P, K = prox == "iso", 2, 3, 4
    need_h = variant != "noh" and M != 256   # 256 x 256: the fused lane-native trajectory (no h_bar)
    kw = dict(need_y=variant != "drop", need_rho=variant != "drop")
    y, hs, lams, rhos = make_case(B, P, N, M, B, P, ("rand", 5, 5), 0.0041, 0.021, K, iso, 1 if iso else B * P)
    xbar = seeded_xbar(y.shape)
    sfx = "_iso" if iso else ""
    paths = {32: ("2pass" + sfx, "sweep_2pass" + sfx), 24: ("runtime", "sweep_runtime" + sfx), 256: ("fused", "sweep_2pass")}[M]
    with _lib.option("MIN_PLANES", 0):
        assert _lib.query_grouped_paths(M, N, iso, 5, B * P, B * P, flags=_lib.REC_HBAR if need_h else 0) == paths, cid
        _lib.profile_reset()
        _lib.profile_enable(True)
        try:
            if call == "replay":
                run_recorded(dev, y, hs, B, P, lams, rhos, iso, K, xbar, need_h=need_h, **kw)
            else:
                run_combined(dev, y, hs, B, P, lams, rhos, iso, K, xbar, need_h=need_h, **kw)
        finally:
            _lib.profile_enable(False)
    c = {name: _lib.profile_get(cls)[1] for cls, name in _lib.KERNEL_CLASSES.items()}
    return tuple(c.get(name, 0) for name in CLASSES)


@pytest.mark.parametrize("cid", sorted(GROUPED_COUNTS))
def test_grouped_launch_counts(dev, cid):
    got = grouped_launch_counts(dev, cid)
    assert got == GROUPED_COUNTS[cid], f"{cid}: launches per class {dict(zip(CLASSES, got))}"


# ---- d. autograd ----------------------------------------------------------------------------------------------------
def test_autograd_entry(dev):
    B, P, N, M, gb, gp, psf, lam, rho, K, iso, nparam, _ = CASES[0]
    y, hs, lams, rhos = make_case(B, P, N, M, gb, gp, psf, lam, rho, K, iso, nparam)
    xbar = seeded_xbar(y.shape)
    rho1 = rhos[:1].copy()                                     # one rho for every group, a lambda per group
    yd, lt, rt, h = to_dev(dev, y, hs, gb, gp, lams, rho1)
    ref = admm_deconv.tvd_fft_grouped_backward(yd, torch.from_numpy(xbar).to(dev), lt, rt, h, iso, K)
    yg, lg, rg, hg = (t.clone().requires_grad_(True) for t in (yd, lt, rt, h))
    x = admm_deconv.tvd_fft_grouped_grad(yg, lg, rg, hg, iso, K)
    assert x.requires_grad and torch.equal(x.detach(), ref[0])
    x.backward(torch.from_numpy(xbar).to(dev))
    torch.cuda.synchronize()
    assert hg.grad.shape == (gb, gp, *hs[0].shape) and lg.grad.shape == (gb * gp,) and rg.grad.shape == (1,)
    assert torch.equal(yg.grad, ref[1]) and torch.equal(hg.grad, ref[2]) and torch.equal(lg.grad, ref[3])
    assert torch.equal(rg.grad, ref[4].sum().reshape(1))      # the 1-element rho collects the per-group rho_bar
    # only what requires grad is formed: lambda alone, a Python float rho
    l2 = lt.clone().requires_grad_(True)
    admm_deconv.tvd_fft_grouped_grad(yd, l2, float(rho1[0]), h, iso, K).backward(torch.from_numpy(xbar).to(dev))
    assert torch.equal(l2.grad, ref[3])
    # without grad: the plain call
    plain = admm_deconv.tvd_fft_grouped(yd, lt, rt, h, iso, K)
    out = admm_deconv.tvd_fft_grouped_grad(yd, lt, rt, h, iso, K)
    assert not out.requires_grad and torch.equal(out, plain)
    with torch.no_grad():
        assert torch.equal(admm_deconv.tvd_fft_grouped_grad(yg, lg, rg, hg, iso, K), plain)
    with pytest.raises(NotImplementedError, match="adjoint"):
        admm_deconv.tvd_fft_grouped(yg, lt, rt, h, iso, K)
