"""CPU: tests/grouped_oracle.py (the yardstick of the grouped GPU tests) against oracle_np -- plane by plane where the
groups differ (anisotropic planes are independent solves), and on the whole batch with one group."""
import numpy as np
import pytest

import oracle_np
from admm_deconv import synth
from grouped_oracle import group_of, tvd_fft_grouped

REL = 1e-12


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _psfs(rng, G, kw, kh):
    hs = [rng.random((kw, kh)) for _ in range(G)]
    return [(h / h.sum()).astype(np.float32) for h in hs]


def _batch(B, P, N, M, hs, gb, gp):
    y = np.empty((B, P, N, M), np.float32)
    for b in range(B):
        for p in range(P):
            h = None if hs is None else hs[group_of(b, p, gb, gp)]
            y[b, p] = synth.make_batch(1, M, N, h, P=1, g0=7 + b * P + p)[0, 0]
    return y


@pytest.mark.parametrize("B,P,N,M,gb,gp,nparam", [(3, 2, 16, 8, 3, 1, 3), (2, 3, 16, 8, 2, 3, 6), (2, 2, 12, 10, 1, 2, 1)])
def test_anisotropic_groups_are_independent_plane_solves(B, P, N, M, gb, gp, nparam):
    rng = np.random.default_rng(B * 1000 + N + M + 5)
    G = gb * gp
    hs = _psfs(rng, G, 2, 3)
    y = _batch(B, P, N, M, hs, gb, gp)
    lam = np.float32(0.05) * (1 + 0.25 * np.arange(nparam, dtype=np.float32))
    rho = np.float32(0.3) * (1 + 0.5 * np.arange(nparam, dtype=np.float32))
    st = {}
    x = oracle_np.to_c(tvd_fft_grouped(oracle_np.from_c(y), lam, rho, [oracle_np.psf_from_c(h) for h in hs], gb, gp,
                                       False, 5, stats=st))
    assert oracle_np.prox_active_fraction(st) > 0.05
    for b in range(B):
        for p in range(P):
            g = group_of(b, p, gb, gp)
            gs = g if nparam > 1 else 0
            for f in (oracle_np.tvd_fft_literal, oracle_np.tvd_fft_spectral):
                ref = oracle_np.to_c(f(oracle_np.from_c(y[b:b + 1, p:p + 1]), lam[gs], rho[gs],
                                       oracle_np.psf_from_c(hs[g]), False, 5))
                assert _rel(x[b, p], ref[0, 0]) <= REL, (b, p, f.__name__)


@pytest.mark.parametrize("iso", [False, True])
@pytest.mark.parametrize("psf", [True, False])
def test_one_group_is_the_reference_batch_solve(iso, psf):
    rng = np.random.default_rng(11)
    B, P, N, M = 2, 3, 10, 12
    hs = _psfs(rng, 1, 3, 4) if psf else None
    y = _batch(B, P, N, M, hs, 1, 1)
    lam, rho = np.float32(0.05), np.float32(0.3)
    st, st_ref = {}, {}
    x = tvd_fft_grouped(oracle_np.from_c(y), lam, rho, None if hs is None else [oracle_np.psf_from_c(hs[0])], 1, 1, iso,
                        6, stats=st)
    ref = oracle_np.tvd_fft_literal(oracle_np.from_c(y), lam, rho, None if hs is None else oracle_np.psf_from_c(hs[0]),
                                    iso, 6, stats=st_ref)
    assert _rel(x, ref) <= REL
    assert st == st_ref and oracle_np.prox_active_fraction(st) > 0.05


def test_isotropic_couples_planes_of_different_groups():
    """The BT norm sums over every plane of the call: a grouped isotropic solve is NOT the per-plane solves."""
    rng = np.random.default_rng(3)
    B, P, N, M = 2, 2, 8, 8
    hs = _psfs(rng, 4, 3, 2)
    y = _batch(B, P, N, M, hs, 2, 2)
    hj = [oracle_np.psf_from_c(h) for h in hs]
    x = oracle_np.to_c(tvd_fft_grouped(oracle_np.from_c(y), 0.05, 0.3, hj, 2, 2, True, 5))
    alone = oracle_np.to_c(oracle_np.tvd_fft_literal(oracle_np.from_c(y[:1, :1]), 0.05, 0.3, hj[0], True, 5))
    assert _rel(x[0, 0], alone[0, 0]) > 1e-3
    with pytest.raises(AssertionError):
        tvd_fft_grouped(oracle_np.from_c(y), [0.05, 0.06, 0.07, 0.08], 0.3, hj, 2, 2, True, 5)
