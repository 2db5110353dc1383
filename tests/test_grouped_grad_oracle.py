"""CPU: the differentiable grouped oracle (tests/grouped_oracle_torch.py) pinned against the numpy grouped oracle's
forward and, group by group, against the single-PSF gradient oracle (oracle/oracle_torch.py)."""
import numpy as np
import pytest

import oracle_np
import oracle_torch
from grouped_oracle import tvd_fft_grouped as oracle_grouped
from grouped_oracle_torch import group_of, tvd_fft_grouped_grads
from test_gpu_grouped import make_case

TOL = 1e-10

# (B, P, N, M, gb, gp, PSF, lambda, rho, K, isotropic, nparam)
CASES = [
    (3, 2, 16, 8, 3, 1, ("rand", 3, 2), 0.05, 0.3, 5, False, 3),      # per image
    (2, 3, 16, 8, 1, 3, ("rand", 3, 2), 0.05, 0.3, 5, False, 3),      # per channel: a group's planes are strided
    (3, 2, 16, 8, 3, 1, ("rand", 3, 2), 0.05, 0.3, 5, False, 1),      # one pair, three PSFs
    (2, 2, 16, 16, 2, 2, None, 0.05, 0.02, 6, False, 4),              # no PSF
    (2, 3, 15, 9, 2, 3, ("rand", 4, 4), 0.02, 0.1, 4, False, 6),      # odd sides, even PSF
    (2, 3, 16, 8, 2, 3, ("rand", 3, 2), 0.05, 0.3, 5, True, 1),       # isotropic: coupled over every plane
]


def _cid(c):
    return f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-g{c[4]}x{c[5]}-n{c[11]}{'-iso' if c[10] else ''}"


def _inputs(case):
    B, P, N, M, gb, gp, psf, lam, rho, K, iso, nparam = case
    y, hs, lams, rhos = make_case(B, P, N, M, gb, gp, psf, lam, rho, K, iso, nparam)
    xbar = np.random.default_rng(17).standard_normal(y.shape)
    return y.astype(np.float64), None if hs is None else [h.astype(np.float64) for h in hs], lams, rhos, xbar


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("case", CASES, ids=[_cid(c) for c in CASES])
def test_forward_is_the_numpy_grouped_oracle(case):
    B, P, N, M, gb, gp, psf, lam, rho, K, iso, nparam = case
    y, hs, lams, rhos, xbar = _inputs(case)
    st = {}
    x = tvd_fft_grouped_grads(y, lams, rhos, hs, gb, gp, iso, K, xbar, stats=st)[0]
    st_np = {}
    ref = oracle_np.to_c(oracle_grouped(oracle_np.from_c(y), lams, rhos,
                                        None if hs is None else [oracle_np.psf_from_c(h) for h in hs], gb, gp, iso, K,
                                        stats=st_np))
    assert relerr(x, ref) <= TOL
    assert np.allclose(st["prox_active"], st_np["prox_active"], atol=1e-12) and max(st["prox_active"]) > 0


@pytest.mark.parametrize("case", [c for c in CASES if not c[10]], ids=[_cid(c) for c in CASES if not c[10]])
def test_group_gradients_are_the_single_oracles(case):
    """Anisotropic planes are independent: y_bar, h_bar_g, lambda_bar_g and rho_bar_g of the grouped oracle are the
    single oracle's on group g's planes alone; with one (lambda, rho) pair the entry is the sum over the groups."""
    B, P, N, M, gb, gp, psf, lam, rho, K, iso, nparam = case
    y, hs, lams, rhos, xbar = _inputs(case)
    G = gb * gp
    x, yb, hb, lb, rb = tvd_fft_grouped_grads(y, lams, rhos, hs, gb, gp, False, K, xbar)
    assert lb.shape == rb.shape == (nparam,) and (hs is None or hb.shape == (G, *hs[0].shape))
    lsum, rsum = 0.0, 0.0
    for g in range(G):
        sel = [(b, p) for b in range(B) for p in range(P) if group_of(b, p, gb, gp) == g]
        assert len(sel) == B * P // G
        yg = np.stack([y[b, p] for b, p in sel])[:, None]
        xg = np.stack([xbar[b, p] for b, p in sel])[:, None]
        gs = g if nparam > 1 else 0
        x1, yb1, hb1, lb1, rb1 = oracle_torch.tvd_fft_grads(yg, lams[gs], rhos[gs], None if hs is None else hs[g], False,
                                                            K, xg)
        for i, (b, p) in enumerate(sel):
            assert relerr(x[b, p], x1[i, 0]) <= TOL
            assert relerr(yb[b, p], yb1[i, 0]) <= TOL
        if hs is not None:
            assert relerr(hb[g], hb1) <= TOL
        if nparam > 1:
            assert abs(lb[g] - lb1) <= TOL * abs(lb1) and abs(rb[g] - rb1) <= TOL * abs(rb1)
        lsum, rsum = lsum + lb1, rsum + rb1
    if nparam == 1:
        assert abs(lb[0] - lsum) <= TOL * abs(lsum) and abs(rb[0] - rsum) <= TOL * abs(rsum)
