"""GPU: the resumable solve (tvd_fft_state / tvd_fft_tol, admm_tvd_forward_state_dev_f32) against the fp64 state oracle
(tests/state_oracle.py) on synth inputs.

Bounds.  x: parity.assert_parity (per-plane rel-L2 <= 1e-5, max-abs guard).  s_K: per-plane rel-L2 (both channels of a
plane) <= max(1e-5, the error of the oracle's own float32 evaluation on the same inputs), factor 1 -- s is a difference
of x, so its relative error is not that of x.  Residual norms: |r| and pri relative to pri, |d| and dual relative to
dual (the scales the stopping rule uses them at), <= max(1e-5, the float32 evaluation's error in the same measure).
Every case asserts a live prox (>= 1 % of the oracle's z_k non-zero).  With ADMM_STATE_PARITY_LOG set to a file name,
every case appends its figures there as JSON lines (profiles/state_parity.jsonl was written that way)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import admm_deconv
import parity
import state_oracle as so
from admm_deconv import _lib, synth

pytestmark = pytest.mark.gpu

LAM, RHO = synth.LAMBDA, synth.RHO
K = 12
SPLITS = [(1, 1), (2, 3), (5, 7), (1, 11)]

# name: (M, N, B, P, PSF size or 0, PSF sigma, isotropic)
CASES = {
    "fused256_psf15": (256, 256, 2, 1, 15, 2.5, False),
    "fused256_nopsf": (256, 256, 2, 1, 0, 0.0, False),
    "2pass_64": (64, 64, 2, 1, 9, 1.2, False),
    "2pass_32x128": (32, 128, 2, 1, 5, 1.0, False),
    "2pass_16x8_wrap": (16, 8, 2, 1, 3, 0.8, False),
    "runtime_40x30": (40, 30, 2, 1, 5, 1.0, False),
    "runtime_33x27": (33, 27, 2, 1, 5, 1.0, False),
    "runtime_96_smooth_shape": (96, 96, 1, 1, 9, 1.2, False),
    "iso_64_b3p1": (64, 64, 3, 1, 9, 1.2, True),
    "iso_64_b2p3": (64, 64, 2, 3, 9, 1.2, True),
    "iso_40x30_b3p1": (40, 30, 3, 1, 5, 1.0, True),
    "iso_40x30_b2p3": (40, 30, 2, 3, 5, 1.0, True),
}


# the path each family of cases runs (the GPU tests lift the plane-count rule, tests/conftest.py)
PATHS = {"fused256": "fused", "2pass": "2pass", "runtime": "runtime", "iso_64": "2pass_iso", "iso_40x30": "runtime"}


def expected_path(name):
    return next(v for k, v in PATHS.items() if name.startswith(k))


@functools.lru_cache(maxsize=None)
def inputs(name):
    M, N, B, P, k, sig, iso = CASES[name]
    psf = synth.gaussian_psf(k, sig) if k else None
    y = synth.make_batch(B, M, N, psf, P=P)
    return y, psf, iso


@functools.lru_cache(maxsize=None)
def oracle(name, k, lam=LAM, start=None):
    """(fp64 result, float32-evaluation result) of k iterations; start = (k0, lam0): from the state of k0 iterations at
    lam0 (each evaluation from its own state).  Computed once per argument tuple and shared; never modified."""
    y, psf, iso = inputs(name)
    s64 = s32 = None
    if start is not None:
        a, b = oracle(name, start[0], start[1])
        s64, s32 = a["state"], b["state"]
    r64 = so.solve(y, lam, RHO, psf, iso, k, s64)
    r32 = so.solve(y, lam, RHO, psf, iso, k, s32, dtype=np.float32)
    return r64, r32


def dev_inputs(name, dev, lam=LAM):
    y, psf, iso = inputs(name)
    return (torch.from_numpy(y).to(dev), torch.tensor([lam], dtype=torch.float32, device=dev),
            torch.tensor([RHO], dtype=torch.float32, device=dev), None if psf is None else torch.from_numpy(psf).to(dev), iso)


def plane_rel(got, ref):
    """worst per-plane rel-L2 of a state (B, P, 2, N, M)."""
    g = np.asarray(got, np.float64).reshape(got.shape[0] * got.shape[1], -1)
    r = np.asarray(ref, np.float64).reshape(g.shape)
    return max(np.linalg.norm(g[i] - r[i]) / max(np.linalg.norm(r[i]), 1e-300) for i in range(g.shape[0]))


def resid_err(got, ref):
    """(|r|, pri) errors relative to pri and (|d|, dual) errors relative to dual: the worst over planes of each."""
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.array([(np.abs(g[..., 0] - r[..., 0]) / r[..., 2]).max(), (np.abs(g[..., 1] - r[..., 1]) / r[..., 3]).max(),
                     (np.abs(g[..., 2] - r[..., 2]) / r[..., 2]).max(), (np.abs(g[..., 3] - r[..., 3]) / r[..., 3]).max()])


def log(**rec):
    path = os.environ.get("ADMM_STATE_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def check_against_oracle(name, what, x, s, resid, r64, r32, **extra):
    """x, s_K and the residual norms of a library call against the oracle's, with the module's bounds."""
    parity.assert_prox_active(so.prox_fraction(r64), f"{name} {what}", linear_only=False)
    print(f"{name} {what}: prox active {so.prox_fraction(r64):.3f}")
    e_s, b_s = plane_rel(s.cpu().numpy(), r64["state"]), max(1e-5, plane_rel(r32["state"], r64["state"]))
    e_r, b_r = resid_err(resid.cpu().numpy(), r64["resid"]), np.maximum(1e-5, resid_err(r32["resid"], r64["resid"]))
    print(f"{name} {what}: s rel-L2 {e_s:.3e} (bound {b_s:.3e}); resid errors {e_r} (bounds {b_r})")
    log(case=name, check=what, s_rel_l2=e_s, s_bound=b_s, resid_err=e_r.tolist(), resid_bound=b_r.tolist(), **extra)
    parity.assert_parity(x.cpu().numpy(), r64["x"], what=f"{name} {what} x")
    assert e_s <= b_s, f"{name} {what}: s_K rel-L2 {e_s:.3e} > {b_s:.3e}"
    assert (e_r <= b_r).all(), f"{name} {what}: residual errors {e_r} > {b_r}"


def same_path_options(M, N, iso, kh, planes):
    """Library options under which the plain forward takes the state call's path."""
    want = _lib.query_state_path(M, N, iso, kh, planes)
    for opts in ({}, {"FUSED": 0}, {"SMOOTH": 0, "RESIDENT": 0}):
        old = {k: _lib.get_option(k) for k in opts}
        try:
            for k, v in opts.items():
                _lib.set_option(k, v)
            if _lib.query_paths(M, N, iso, kh, planes=planes)[0] == want:
                return opts
        finally:
            for k, v in old.items():
                _lib.set_option(k, v)
    raise AssertionError(f"no options give the plain forward the path {want}")


@pytest.mark.parametrize("name", ["fused256_psf15", "2pass_64", "2pass_32x128", "runtime_33x27", "iso_64_b2p3",
                                  "iso_40x30_b3p1"])
def test_pass_through_is_the_plain_forward(dev, name):
    y, lam, rho, h, iso = dev_inputs(name, dev)
    B, P, N, M = y.shape
    opts = same_path_options(M, N, iso, 0 if h is None else h.shape[1], B * P)
    old = {k: _lib.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            _lib.set_option(k, v)
        ref = admm_deconv.tvd_fft(y, lam, rho, h, iso, K)
    finally:
        for k, v in old.items():
            _lib.set_option(k, v)
    x, s, r = admm_deconv.tvd_fft_state(y, lam, rho, h, iso, K, want_state=False, want_residuals=False)
    assert s is None and r is None
    assert torch.equal(x, ref)


@pytest.mark.parametrize("name", list(CASES))
def test_cold_state_and_residuals(dev, name):
    y, lam, rho, h, iso = dev_inputs(name, dev)
    r64, r32 = oracle(name, K)
    B, P, N, M = y.shape
    assert _lib.query_state_path(M, N, iso, 0 if h is None else h.shape[1], B * P) == expected_path(name)
    x, s, resid = admm_deconv.tvd_fft_state(y, lam, rho, h, iso, K)
    assert s.shape == (*y.shape[:2], 2, *y.shape[2:]) and resid.shape == (*y.shape[:2], 4)
    check_against_oracle(name, "cold", x, s, resid, r64, r32)
    # the state without the residuals and the residuals without the state are the same numbers
    x2, s2, none = admm_deconv.tvd_fft_state(y, lam, rho, h, iso, K, want_residuals=False)
    x3, none3, resid3 = admm_deconv.tvd_fft_state(y, lam, rho, h, iso, K, want_state=False)
    assert none is None and none3 is None
    assert torch.equal(x2, x) and torch.equal(s2, s) and torch.equal(x3, x) and torch.equal(resid3, resid)


@pytest.mark.parametrize("split", SPLITS, ids=lambda s: f"{s[0]}+{s[1]}")
@pytest.mark.parametrize("name", list(CASES))
def test_composition(dev, name, split):
    a, b = split
    y, lam, rho, h, iso = dev_inputs(name, dev)
    r64, r32 = oracle(name, a + b)
    _, s_a, _ = admm_deconv.tvd_fft_state(y, lam, rho, h, iso, a, want_residuals=False)
    keep = s_a.clone()
    x, s, resid = admm_deconv.tvd_fft_state(y, lam, rho, h, iso, b, state=s_a)
    assert torch.equal(s_a, keep)
    whole_x, whole_s, _ = admm_deconv.tvd_fft_state(y, lam, rho, h, iso, a + b, want_residuals=False)
    dx, ds = float((x - whole_x).abs().max()), float((s - whole_s).abs().max())
    print(f"{name} {a}+{b}: split vs whole max-abs x {dx:.3e}, s {ds:.3e}")   # logged, not bounded
    check_against_oracle(name, f"split {a}+{b}", x, s, resid, r64, r32, split_vs_whole_x=dx, split_vs_whole_s=ds)


@pytest.mark.parametrize("name", list(CASES))
def test_warm_start_under_another_lambda(dev, name):
    y, lam, rho, h, iso = dev_inputs(name, dev)
    _, lam2, _, _, _ = dev_inputs(name, dev, 2 * LAM)
    r64, r32 = oracle(name, 7, 2 * LAM, (5, LAM))
    _, s5, _ = admm_deconv.tvd_fft_state(y, lam, rho, h, iso, 5, want_residuals=False)
    x, s, resid = admm_deconv.tvd_fft_state(y, lam2, rho, h, iso, 7, state=s5)
    check_against_oracle(name, "warm 5 at lambda + 7 at 2 lambda", x, s, resid, r64, r32)


@pytest.mark.parametrize("iso,stop", [(False, 40), (True, 30)])
def test_tol_stops_where_the_oracle_stops(dev, iso, stop):
    psf = synth.gaussian_psf(9, 1.2)
    y = synth.make_batch(2, 64, 64, psf)
    ref, iters, _ = so.solve_tol(y, LAM, RHO, psf, iso, 100, 0.0, 1e-2, 10)
    assert iters == stop
    yt, ht = torch.from_numpy(y).to(dev), torch.from_numpy(psf).to(dev)
    x, s, it, resid = admm_deconv.tvd_fft_tol(yt, LAM, RHO, ht, iso, 100, eps_rel=1e-2, check_every=10)
    assert it == stop
    parity.assert_parity(x.cpu().numpy(), ref["x"], what=f"tol iso={iso}")
    assert so.stop_met(resid.cpu().numpy(), 64, 64, 0.0, 1e-2)
    assert s.shape == (2, 1, 2, 64, 64)


def test_tol_runs_maxit_in_blocks(dev):
    psf = synth.gaussian_psf(9, 1.2)
    y = synth.make_batch(2, 64, 64, psf)
    yt, ht = torch.from_numpy(y).to(dev), torch.from_numpy(psf).to(dev)
    calls = []
    real = admm_deconv.ops.tvd_fft_state

    def spy(*a, **k):
        calls.append(a[5])
        return real(*a, **k)

    admm_deconv.ops.tvd_fft_state = spy
    try:
        x, s, it, resid = admm_deconv.tvd_fft_tol(yt, LAM, RHO, ht, False, 23, eps_rel=0.0, check_every=10)
    finally:
        admm_deconv.ops.tvd_fft_state = real
    assert it == 23 and calls == [10, 10, 3]
    whole, ws, _ = admm_deconv.tvd_fft_state(yt, LAM, RHO, ht, False, 23, want_residuals=False)
    parity.assert_parity(x.cpu().numpy(), so.solve(y, LAM, RHO, psf, False, 23)["x"], what="tol 23")
    print(f"tol 10+10+3 vs 23: max-abs x {float((x - whole).abs().max()):.3e}")


@pytest.mark.parametrize("name", ["fused256_psf15", "2pass_64", "runtime_33x27", "iso_64_b2p3"])
def test_deterministic_and_inputs_untouched(dev, name):
    y, lam, rho, h, iso = dev_inputs(name, dev)
    y0 = y.clone()
    _, s5, _ = admm_deconv.tvd_fft_state(y, lam, rho, h, iso, 5, want_residuals=False)
    s5_0 = s5.clone()
    a = admm_deconv.tvd_fft_state(y, lam, rho, h, iso, 7, state=s5)
    b = admm_deconv.tvd_fft_state(y, lam, rho, h, iso, 7, state=s5)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(y, y0) and torch.equal(s5, s5_0)


@pytest.mark.parametrize("M", [256, 64])
def test_anisotropic_planes_do_not_depend_on_the_batch(dev, M):
    psf = synth.gaussian_psf(9, 1.2)
    y = torch.from_numpy(synth.make_batch(3, M, M, psf)).to(dev)
    h = torch.from_numpy(psf).to(dev)
    _, s3, _ = admm_deconv.tvd_fft_state(y, LAM, RHO, h, False, 3, want_residuals=False)
    x3, t3, r3 = admm_deconv.tvd_fft_state(y, LAM, RHO, h, False, 4, state=s3)
    _, s1, _ = admm_deconv.tvd_fft_state(y[:1], LAM, RHO, h, False, 3, want_residuals=False)
    x1, t1, r1 = admm_deconv.tvd_fft_state(y[:1], LAM, RHO, h, False, 4, state=s1)
    assert torch.equal(x3[:1], x1) and torch.equal(t3[:1], t1) and torch.equal(r3[:1], r1)


def test_refuses_autograd_and_bad_states(dev):
    y, lam, rho, h, iso = dev_inputs("2pass_64", dev)
    with pytest.raises(ValueError):
        admm_deconv.tvd_fft_state(y.clone().requires_grad_(), lam, rho, h, iso, 3)
    with torch.no_grad():
        admm_deconv.tvd_fft_state(y.clone().requires_grad_(), lam, rho, h, iso, 3)
    with pytest.raises(ValueError):
        admm_deconv.tvd_fft_state(y, lam, rho, h, iso, 0)
    with pytest.raises(ValueError):
        admm_deconv.tvd_fft_state(y, lam, rho, h, iso, 3, state=torch.zeros(2, 1, 2, 64, 32, device=dev))
