"""CPU: the fp64 oracle of the resumable solve (tests/state_oracle.py) against oracle_np's own loop, its composition
and residual identities, and the stopping points the GPU tests of tvd_fft_tol rely on."""
import numpy as np
import pytest

import oracle_np
import state_oracle as so
from admm_deconv import synth

LAM, RHO = synth.LAMBDA, synth.RHO
PSF = synth.gaussian_psf(9, 1.2)


@pytest.fixture(scope="module")
def smoke_batch():
    return synth.make_batch(2, 64, 64, PSF)


@pytest.mark.parametrize("iso", [False, True])
def test_cold_start_is_the_literal_loop(smoke_batch, iso):
    y = smoke_batch
    ref = oracle_np.to_c(oracle_np.tvd_fft_literal(oracle_np.from_c(np.asarray(y, np.float64)), np.float32(LAM),
                                                   np.float32(RHO), oracle_np.psf_from_c(PSF), iso, 12))
    got = so.solve(y, LAM, RHO, PSF, iso, 12)
    assert np.abs(got["x"] - ref).max() == 0.0
    assert so.prox_fraction(got) >= 0.01


@pytest.mark.parametrize("iso", [False, True])
def test_split_solve_is_the_whole_solve(smoke_batch, iso):
    y = smoke_batch
    whole = so.solve(y, LAM, RHO, PSF, iso, 12)
    a = so.solve(y, LAM, RHO, PSF, iso, 5)
    b = so.solve(y, LAM, RHO, PSF, iso, 7, state=a["state"])
    assert np.abs(b["x"] - whole["x"]).max() == 0.0
    assert np.abs(b["state"] - whole["state"]).max() == 0.0
    assert np.abs(b["resid"] - whole["resid"]).max() == 0.0


@pytest.mark.parametrize("iso", [False, True])
def test_state_layout_is_D_ops_channels(smoke_batch, iso):
    """s_1 of a cold start is D x_1: channel 0 of a plane the difference along N, channel 1 along M."""
    y = smoke_batch
    got = so.solve(y, LAM, RHO, PSF, iso, 1)
    x = got["x"]
    assert np.abs(got["state"][:, :, 0] - (x - np.roll(x, 1, axis=2))).max() <= 1e-15
    assert np.abs(got["state"][:, :, 1] - (x - np.roll(x, 1, axis=3))).max() <= 1e-15
    xj = oracle_np.from_c(x).transpose(0, 1, 3, 2)
    assert np.abs(so.state_from_c(got["state"]) - oracle_np.D_op(xj)).max() <= 1e-15
    assert np.array_equal(so.state_to_c(so.state_from_c(got["state"])), got["state"])


@pytest.mark.parametrize("iso", [False, True])
def test_primal_residual_identity(smoke_batch, iso):
    got = so.solve(smoke_batch, LAM, RHO, PSF, iso, 12)
    assert np.abs(got["resid"][..., 0] - got["r_alt"]).max() <= 1e-12


@pytest.mark.parametrize("iso,stop,last_miss", [(False, 40, 30), (True, 30, 20)])
def test_stopping_points_of_the_smoke_batch(smoke_batch, iso, stop, last_miss):
    """eps_rel = 1e-2, eps_abs = 0, check_every = 10: the oracle stops at 40 (anisotropic) / 30 (isotropic) iterations,
    and at the two deciding blocks every ratio that decides the global stop is at least 3 % from the threshold -- the
    condition on the inputs that keeps the iteration count stable against fp32 rounding on the GPU."""
    eps = 1e-2
    res, iters, hist = so.solve_tol(smoke_batch, LAM, RHO, PSF, iso, 100, 0.0, eps, 10)
    assert iters == stop
    miss, hit = hist[last_miss // 10 - 1], hist[stop // 10 - 1]
    ratios = lambda r: np.stack([r[..., 0] / r[..., 2], r[..., 1] / r[..., 3]])   # noqa: E731
    # the block before the stop fails through at least one ratio, every failing ratio by 3 % or more; ratios that pass
    # there do not decide (the stop needs all of them)
    rm = ratios(miss)
    assert (rm > eps).any() and rm[rm > eps].min() >= 1.03 * eps
    assert all(ratios(h).max() >= 1.03 * eps for h in hist[:-1])   # every earlier block misses as clearly
    assert ratios(hit).max() <= 0.97 * eps
    # the blocked run is the whole run
    whole = so.solve(smoke_batch, LAM, RHO, PSF, iso, stop)
    assert np.abs(whole["x"] - res["x"]).max() == 0.0
