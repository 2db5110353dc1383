"""GPU: every compiled FFT plan of admm_smooth.hip and the runtime factorisations of admm_generic.hip, per bin.

Each of the 41 compiled lengths runs as a line length (9 x L) and as a column length (L x 18) in both radix orders; the
runtime plans run single radices, prime powers, lengths with two direct-DFT factors, primes and the lengths near 4096 in
both roles (tests/spectral_parity.py lists the cases and says why these shapes).  Inputs are white noise, B = 2, P = 1,
K = 3, lambda = 0.05, rho = 0.1, a 3 x 3 PSF; the CU-resident solve is off, so that the 2-pass kernels run.  Every case
asserts the path it was designed for (admm_query_paths), tests/parity.py's criterion unchanged against the fp64 oracle
(tests/state_oracle.py), and the per-bin bound c_f * e of tests/spectral_parity.py.  With ADMM_LENGTH_SWEEP_LOG set to
a file name every case appends its figures there as JSON lines (profiles/length_sweep_parity.jsonl was written that
way; the constants c_f come from it)."""
import json
import os
import time

import numpy as np
import pytest
import torch

import admm_deconv
import oracle_torch
import parity
import spectral_parity as sp
from admm_deconv import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _two_pass_kernels(dev):
    with _lib.option("RESIDENT", 0):
        yield


def log(**rec):
    path = os.environ.get("ADMM_LENGTH_SWEEP_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def _options(case):
    return _lib.option("SMOOTH", 1 if case.smooth is None else case.smooth)


def _dev_inputs(case, dev):
    y, lam, rho, h = sp.inputs(case)
    return y, lam, rho, h, torch.from_numpy(y).to(dev), None if h is None else torch.from_numpy(h).to(dev)


@pytest.mark.parametrize("case", sp.forward_cases(), ids=lambda c: c.id)
def test_length_sweep_forward(dev, case):
    y, lam, rho, h, yt, ht = _dev_inputs(case, dev)
    r64, r32 = sp.oracle(case)
    parity.assert_prox_active(sp.prox_fraction(case), case.id)
    with _options(case):
        path = _lib.query_paths(case.M, case.N, case.iso, 0 if h is None else h.shape[1], planes=case.B)[0]
        assert path == case.path, f"{case.id}: runs the {path} path, designed for {case.path}"
        torch.cuda.synchronize()
        t0 = time.perf_counter()   # one solve per case (the 2039-point primes take seconds): its first-call costs included
        x = admm_deconv.tvd_fft(yt, lam, rho, ht, case.iso, sp.K)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
    got = x.cpu().numpy()
    e, g = sp.yardstick(case), sp.bin_error(got, r64["x"])
    c = sp.BOUND_FACTOR[case.family]
    print(f"{case.id} [{case.family}]: per-bin e {e:.3e} g {g:.3e} g/e {g / e:.2f} solve {ms:.1f} ms")
    order = None
    if case.family == "compiled_column":   # the radix order this call's column plan runs in (admm_smooth.hip column_asc)
        order = "asc" if case.smooth == 2 or (case.smooth is None and case.L in sp.COL_ASC_LENGTHS) else "desc"
    log(case=case.id, family=case.family, role=case.role, L=case.L, column_order=order, N=case.N, M=case.M, B=case.B,
        iso=case.iso, smooth=case.smooth, path=path, R=case.R, e=e, g=g, ratio=g / e, c=c, bound=sp.bound(case), solve_ms=ms)
    parity.assert_parity(got, r64["x"], what=case.id)
    assert g <= sp.bound(case), (f"{case.id}: per-bin error {g:.3e} > {sp.bound(case):.3e} = c x e "
                                 f"(e {e:.3e}, {case.family}, R {case.R})")


@pytest.mark.parametrize("need_h", [False, True], ids=["noh", "hbar"])
@pytest.mark.parametrize("case", sp.adjoint_cases(), ids=lambda c: c.id)
def test_length_sweep_adjoint(dev, case, need_h):
    """Bounds of tests/test_gpu_smooth.py: 1e-3 relative on y_bar, h_bar, lambda_bar and rho_bar against fp64 autograd of
    the oracle.  The per-bin figure of y_bar is logged only: gradients jump at mask flips."""
    y, lam, rho, h, yt, ht = _dev_inputs(case, dev)
    xbar = np.random.default_rng(case.seed + 1).standard_normal(y.shape).astype(np.float32)
    with _options(case):
        path = _lib.query_paths(case.M, case.N, False, h.shape[1], mode=_lib.MODE_BACKWARD, want_hbar=need_h,
                                want_rho=True, planes=case.B)[0]
        assert path == case.path, f"{case.id}: the forward runs the {path} path, designed for {case.path}"
        t0 = time.perf_counter()
        x, yb, hb, lb, rb = admm_deconv.tvd_fft_backward(yt, torch.from_numpy(xbar).to(dev), lam, rho, ht, False, sp.K,
                                                         need_h=need_h)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
    x0, yb0, hb0, lb0, rb0 = oracle_torch.tvd_fft_grads(y.astype(np.float64), np.float32(lam), np.float32(rho),
                                                        h.astype(np.float64), False, sp.K, xbar)
    yb = yb.cpu().numpy()
    e_y = np.linalg.norm(yb - yb0) / np.linalg.norm(yb0)
    e_l, e_r = abs(float(lb) - lb0) / abs(lb0), abs(float(rb) - rb0) / abs(rb0)
    e_h = float(np.linalg.norm(hb.cpu().numpy() - hb0) / np.linalg.norm(hb0)) if need_h else None
    gb = sp.bin_error(yb, yb0)
    print(f"{case.id} need_h={need_h}: y_bar rel-L2 {e_y:.2e} per-bin {gb:.2e}, lambda_bar {e_l:.2e}, rho_bar {e_r:.2e}, "
          f"h_bar {e_h}; {ms:.1f} ms")
    log(case=case.id, family=case.family, N=case.N, M=case.M, need_h=need_h, path=path, ybar_rel=e_y, ybar_bin=gb,
        lam_rel=e_l, rho_rel=e_r, hbar_rel=e_h, solve_ms=ms)
    parity.assert_parity(x.cpu().numpy(), x0, what=case.id + " x")
    assert e_y < 1e-3 and e_l < 1e-3 and e_r < 1e-3, (e_y, e_l, e_r)
    if need_h:
        assert e_h < 1e-3, e_h
