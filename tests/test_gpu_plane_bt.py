"""GPU: isotropic TV per image plane (isotropic="plane", ADMM_ISO_PLANE) through every layer.

Oracle: tests/plane_bt_oracle.py (the reference's isotropic solve on one plane at a time, fp64); cases:
tests/plane_bt_cases.py; tests/test_plane_bt.py shows without a GPU that the batch-coupled and the anisotropic prox are
at least 1e-2 away on every forward case, so the parity test fails on a library that runs either.  Forward: tests/parity.py
unchanged (1e-5 rel-L2 per plane, 2e-4 max-abs).  Gradients: 1e-3 (x_bar-weighted y_bar and h_bar in rel-L2, lambda_bar and
rho_bar of their value), the figure tests/test_gpu_smooth.py and the length sweep hold gradients to; the adjoint cases sit
at least 1e-5 from the kink of the prox (asserted on the CPU).  With ADMM_PLANE_BT_LOG set to a file name every case
appends its figures there as JSON lines (profiles/plane_bt_parity.jsonl was written that way)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import admm_deconv
import parity
import plane_bt_oracle as pbo
from admm_deconv import _lib, layers, ops
from plane_bt_cases import ADJ_CASES, FWD_2PASS, FWD_CASES, FWD_SEED, K_ADJ, K_FWD, case_id, fwd_K

pytestmark = pytest.mark.gpu

LAM, RHO = pbo.LAM, pbo.RHO
GRAD_TOL = 1e-3


def log(**rec):
    path = os.environ.get("ADMM_PLANE_BT_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _solve(yt, ht, K, iso="plane", lam=LAM, rho=RHO):
    x = admm_deconv.tvd_fft(yt, lam, rho, ht, iso, K)
    torch.cuda.synchronize()
    return x


@pytest.mark.parametrize("case", FWD_CASES, ids=case_id)
def test_forward_parity(dev, case):
    B, P, N, M, k = case
    K = fwd_K(case)
    y, _, h = pbo.inputs(B, P, N, M, k, FWD_SEED)
    st = {}
    ref = pbo.solve_loop(y, LAM, RHO, h, K, stats=st)
    parity.assert_prox_active(st["nonzero"], case_id(case))
    e = pbo.worst_plane_rel(pbo.solve_loop(y, LAM, RHO, h, K, dtype=np.float32), ref)
    path = _lib.query_paths(M, N, "plane", k, planes=B * P)[0]
    assert path == ("2pass" if case in FWD_2PASS else "runtime")
    got = _solve(_t(y, dev), _t(h, dev), K).cpu().numpy()
    g = pbo.worst_plane_rel(got, ref)
    print(f"{case_id(case)} [{path}]: rel-L2 g {g:.3e}, float32 yardstick e {e:.3e}, g/e {g / e:.2f}")
    log(test="forward", case=case_id(case), path=path, K=K, g=g, e=e, ratio=g / e)
    parity.assert_parity(got, ref, what=case_id(case))


@pytest.mark.parametrize("case", [(2, 3, 16, 32, 5), (2, 3, 30, 40, 5)], ids=case_id)
def test_batch_independence_and_determinism(dev, case):
    B, P, N, M, k = case
    y, _, h = pbo.inputs(B, P, N, M, k, FWD_SEED)
    yt, ht = _t(y, dev), _t(h, dev)
    y0 = yt.clone()
    a = _solve(yt, ht, K_FWD)
    b = _solve(yt, ht, K_FWD)
    assert torch.equal(a, b), "two calls must give the same bits"
    assert torch.equal(yt, y0), "y is not modified"
    for bb in range(B):
        for p in range(P):
            one = _solve(yt[bb:bb + 1, p:p + 1].contiguous(), ht, K_FWD)
            assert torch.equal(one[0, 0], a[bb, p]), f"plane ({bb}, {p}) depends on its batch"
    # ... which is what the batch-coupled prox cannot do
    c = _solve(yt, ht, K_FWD, iso=True)
    c1 = _solve(yt[:1, :1].contiguous(), ht, K_FWD, iso=True)
    assert not torch.equal(c[0, 0], c1[0, 0])


def test_launch_shape(dev):
    B, P, N, M, k = (2, 3, 16, 32, 5)
    y, _, h = pbo.inputs(B, P, N, M, k, FWD_SEED)
    yt, ht = _t(y, dev), _t(h, dev)
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        _solve(yt, ht, K_FWD)
    finally:
        _lib.profile_enable(False)
    n = {name: _lib.profile_get(cls)[1] for cls, name in _lib.KERNEL_CLASSES.items()}
    _lib.profile_reset()
    assert n["norm"] == 0 and n["line"] == K_FWD - 1 and n["column"] == K_FWD and n["plane"] == 0, n


def test_plane_chunking(dev):
    """More planes than one launch sequence takes (65,280): consecutive chunks, as for the anisotropic solve."""
    rng = np.random.default_rng(FWD_SEED)
    planes = 65300
    y = _t(rng.standard_normal((planes, 1, 2, 4)).astype(np.float32), dev)
    a = _solve(y, None, 2)
    b = torch.cat([_solve(y[:40000].contiguous(), None, 2), _solve(y[40000:].contiguous(), None, 2)])
    assert torch.equal(a, b)
    assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0


@pytest.mark.parametrize("shape", [(16, 32), (30, 40)], ids=["16x32", "30x40"])
def test_grouped_takes_scalars_per_group(dev, shape):
    N, M = shape
    B = P = 2
    rng = np.random.default_rng(FWD_SEED)
    y = rng.standard_normal((B, P, N, M)).astype(np.float32)
    hs = np.stack([pbo.gaussian_psf(5, s) for s in (0.8, 1.0, 1.3, 1.7)]).reshape(B, P, 5, 5)
    lams = np.array([0.05, 0.03, 0.08, 0.06], np.float32)
    rhos = np.array([0.1, 0.12, 0.07, 0.2], np.float32)
    yt = _t(y, dev)
    x = ops.tvd_fft_grouped(yt, _t(lams, dev), _t(rhos, dev), _t(hs, dev), "plane", K_FWD)
    torch.cuda.synchronize()
    assert _lib.query_grouped_path(M, N, "plane", 5, B * P, 4) == ("2pass" if N == 16 else "runtime")
    for b in range(B):
        for p in range(P):
            g = b * P + p
            one = _solve(yt[b:b + 1, p:p + 1].contiguous(), _t(hs[b, p], dev), K_FWD, lam=float(lams[g]), rho=float(rhos[g]))
            assert torch.equal(one[0, 0], x[b, p]), f"plane ({b}, {p}) is not the single solve with its group's parameters"
    # and a plane is what the oracle says (group 3: its own PSF, lambda and rho)
    ref = pbo.solve_loop(y[1:, 1:], lams[3], rhos[3], hs[1, 1], K_FWD)
    parity.assert_parity(x[1:, 1:].cpu().numpy(), ref, what="grouped plane (1, 1)")


@functools.lru_cache(maxsize=None)
def _adj_oracle(case, seed):
    B, P, N, M, k = case
    y, xbar, h = pbo.inputs(B, P, N, M, k, seed)
    return y, xbar, h, pbo.grads_loop(y, LAM, RHO, h, K_ADJ, xbar)


def _check_grads(what, got, ref, xbar, need_h):
    """got / ref: (x, ybar, hbar, lam_bar, rho_bar).  Returns the measured errors."""
    err = {"x": pbo.worst_plane_rel(got[0], ref[0]), "ybar": pbo.rel_l2(got[1], ref[1]),
           "lam": abs(got[3] - ref[3]) / abs(ref[3]), "rho": abs(got[4] - ref[4]) / abs(ref[4])}
    if need_h and ref[2] is not None:
        err["hbar"] = pbo.rel_l2(got[2], ref[2])
    print(what, {k: f"{v:.2e}" for k, v in err.items()})
    assert err["x"] <= parity.REL_L2_TOL, (what, err)
    for k in ("ybar", "hbar", "lam", "rho"):
        assert err.get(k, 0.0) <= GRAD_TOL, (what, k, err)
    return err


def _np(t):
    return None if t is None else t.detach().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("need_h", [False, True], ids=["noh", "hbar"])
@pytest.mark.parametrize("case,seed", ADJ_CASES, ids=lambda v: case_id(v) if isinstance(v, tuple) else f"s{v}")
def test_adjoint(dev, case, seed, need_h):
    B, P, N, M, k = case
    y, xbar, h, ref = _adj_oracle(case, seed)
    yt, xt, ht = _t(y, dev), _t(xbar, dev), _t(h, dev)
    bwd = "sweep_2pass" if case in FWD_2PASS else "sweep_runtime"
    assert _lib.query_paths(M, N, "plane", k, mode=_lib.MODE_BACKWARD, want_hbar=need_h, want_rho=True, planes=B * P)[1] == bwd
    # the combined call
    x, yb, hb, lb, rb = ops.tvd_fft_backward(yt, xt, LAM, RHO, ht, "plane", K_ADJ, need_h=need_h)
    torch.cuda.synchronize()
    got = (_np(x), _np(yb), _np(hb), float(lb), float(rb))
    err = _check_grads(f"{case_id(case)} backward", got, ref, xbar, need_h)
    log(test="adjoint", case=case_id(case), seed=seed, need_h=need_h, path=bwd, **err)
    # record + replay: the same sweep from the recorded trajectory
    xr, rec = ops.tvd_fft_record(yt, LAM, RHO, ht, "plane", K_ADJ, need_h=need_h)
    yb2, hb2, lb2, rb2 = ops.tvd_fft_backward_recorded(rec, xr, xt)
    torch.cuda.synchronize()
    assert torch.equal(xr, x) and torch.equal(yb2, yb) and torch.equal(lb2, lb) and torch.equal(rb2, rb)
    assert (hb2 is None and hb is None) or torch.equal(hb2, hb)
    # dropping y_bar or rho_bar leaves the other gradients bitwise unchanged
    _, yb3, hb3, lb3, rb3 = ops.tvd_fft_backward(yt, xt, LAM, RHO, ht, "plane", K_ADJ, need_h=need_h, need_y=False)
    assert yb3 is None and torch.equal(lb3, lb) and torch.equal(rb3, rb) and ((hb is None) or torch.equal(hb3, hb))
    _, yb4, hb4, lb4, rb4 = ops.tvd_fft_backward(yt, xt, LAM, RHO, ht, "plane", K_ADJ, need_h=need_h, need_rho=False)
    assert rb4 is None and torch.equal(yb4, yb) and torch.equal(lb4, lb) and ((hb is None) or torch.equal(hb4, hb))


@pytest.mark.parametrize("other", [False, True], ids=["iso0", "iso1"])
def test_replay_with_another_prox_is_refused(dev, other):
    B, P, N, M, k = (2, 3, 16, 32, 5)
    y, xbar, h = pbo.inputs(B, P, N, M, k, 7)
    yt, xt, ht = _t(y, dev), _t(xbar, dev), _t(h, dev)
    x, rec = ops.tvd_fft_record(yt, LAM, RHO, ht, "plane", K_ADJ)
    rec.iso = other
    with pytest.raises(_lib.AdmmError) as ei:
        ops.tvd_fft_backward_recorded(rec, x, xt)
    assert ei.value.code in (_lib.ADMM_E_INVALID, _lib.ADMM_E_WORKSPACE)
    # the recording is kept: its own replay still runs
    rec.iso = "plane"
    yb, _, _, _ = ops.tvd_fft_backward_recorded(rec, x, xt)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(yb).all())


def test_autograd_reproduces_the_adjoint(dev):
    B, P, N, M, k = (2, 3, 16, 32, 5)
    y, xbar, h = pbo.inputs(B, P, N, M, k, 7)
    xt = _t(xbar, dev)
    yt, ht = _t(y, dev).requires_grad_(), _t(h, dev).requires_grad_()
    lam = torch.tensor([LAM], device=dev, requires_grad=True)
    rho = torch.tensor([RHO], device=dev, requires_grad=True)
    x = admm_deconv.tvd_fft(yt, lam, rho, ht, "plane", K_ADJ)
    (x * xt).sum().backward()
    x2, yb, hb, lb, rb = ops.tvd_fft_backward(yt.detach(), xt, lam.detach(), rho.detach(), ht.detach(), "plane", K_ADJ)
    torch.cuda.synchronize()
    assert torch.equal(x.detach(), x2) and torch.equal(yt.grad, yb) and torch.equal(ht.grad, hb)
    assert torch.equal(lam.grad.reshape(()), lb) and torch.equal(rho.grad.reshape(()), rb)


def test_layer_equals_the_op(dev):
    rng = np.random.default_rng(3)
    d = layers.ADMMDeconv((5, 5), 4, iso="plane", device=dev)
    xin = _t(rng.standard_normal((2, 3, 16, 32)).astype(np.float32), dev)
    xbar = _t(rng.standard_normal((2, 3, 16, 32)).astype(np.float32), dev)
    for t in (d.weight, d.lam, d.rho):
        t.requires_grad_()
    out = d(xin)
    (out * xbar).sum().backward()
    d.project()
    x2, _, hb, lb, rb = ops.tvd_fft_backward(xin, xbar, d.lam.detach(), d.rho.detach(), d.weight.detach(), "plane", 4,
                                             need_y=False)
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), x2)
    assert torch.equal(d.weight.grad, hb.reshape(d.weight.shape))
    assert torch.equal(d.lam.grad.reshape(()), lb) and torch.equal(d.rho.grad.reshape(()), rb)


def test_parallel_runs_the_branches_one_by_one(dev):
    rng = np.random.default_rng(4)
    a = layers.ADMMDeconvF2((), 4, 0.1, iso="plane", device=dev)
    b = layers.ADMMDeconvF2((), 4, 0.2, iso="plane", device=dev)
    xin = _t(rng.standard_normal((2, 3, 16, 32)).astype(np.float32), dev)
    par = layers.Parallel(layers.chcat, a, b)
    assert not par._mergeable(xin)
    out = par(xin)
    ref = layers.chcat(a(xin), b(xin))
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
