"""fp64 oracle of the resumable solve (include/admm_deconv.h, admm_tvd_forward_state_dev_f32): the reference loop
(ops.jl:84-92) built from oracle_np's own operators, with the ADMM state going in and coming out.

The state after k iterations is s_k = D x_k + u_{k-1}; z_k = prox(s_k, lambda / rho) and u_k = s_k - z_k follow from it.
In C layout it is (B, P, 2, N, M): plane (b, p) holds D_op's output channels 2b (the difference along dim 2, N) and 2b + 1
(along dim 1, M) of channel-batch p.  `dtype=np.float32` evaluates the same loop with every array rounded to float32
after every operator (the transforms themselves are numpy's): the error of that evaluation against the fp64 one is what
fp32 arithmetic costs this algorithm on these inputs, and bounds the library's distance from the fp64 oracle."""
import numpy as np

import oracle_np as o


def state_to_c(s):
    """(M, N, 2B, P) working array -> (B, P, 2, N, M)."""
    M, N, B2, P = s.shape
    return np.ascontiguousarray(s.reshape(M, N, B2 // 2, 2, P).transpose(2, 4, 3, 1, 0))


def state_from_c(sc):
    """(B, P, 2, N, M) -> (M, N, 2B, P)."""
    B, P, _, N, M = sc.shape
    return np.ascontiguousarray(np.asarray(sc).transpose(4, 3, 0, 2, 1).reshape(M, N, 2 * B, P))


def _plane_norms(a, per_pixel_channels):
    """2-norm per plane (b, p) of a working array: (M, N, 2B, P) with both channels of a plane, or (M, N, B, P)."""
    a = np.asarray(a, np.float64)
    M, N, C, P = a.shape
    B = C // per_pixel_channels
    q = (a * a).reshape(M, N, B, per_pixel_channels, P).sum(axis=(0, 1, 3))   # (B, P)
    return np.sqrt(q)


def solve(y, lam, rho, h=None, iso=False, K=1, state=None, dtype=np.float64):
    """K >= 1 iterations from `state` (C layout; None: zeros) on C-layout inputs y (B, P, N, M), h (kw, kh) or None;
    lam and rho are rounded to float32 as the library takes them.  Returns a dict: x (B, P, N, M), state = s_K
    (B, P, 2, N, M), resid (B, P, 4) = (|r|, |d|, pri, dual) with r = D x_K - z_K, d = rho D^T (z_K - z_{K-1}), pri =
    max(|D x_K|, |z_K|), dual = rho |D^T u_K|; r_alt = |u_K - u_{K-1}| per plane (the residual identity); prox_active:
    the fraction of non-zero z_k per iteration, k = 1..K."""
    assert K >= 1
    cdt = np.complex64 if dtype == np.float32 else np.complex128
    r_ = lambda a: np.asarray(a, dtype)   # noqa: E731  -- round after every operator
    yj = o.from_c(np.asarray(y, np.float64))
    M, N, P, B = yj.shape
    lam = dtype(np.float32(lam))
    rho = dtype(np.float32(rho))
    tau = dtype(lam / rho)
    yp = r_(yj.transpose(0, 1, 3, 2))
    hj = o.psf_from_c(h)
    hj = None if hj is None or np.size(hj) == 0 else np.asarray(hj, np.float64)
    C = r_(o.make_C(M, N, float(rho), hj)[:, :, None, None])
    thresh = o.BT if iso else o.ST
    hty = yp.copy() if hj is None else r_(o.Ht_op(yp, r_(hj)))
    s = np.zeros((M, N, 2 * B, P), dtype) if state is None else r_(state_from_c(np.asarray(state, np.float64)))
    z = r_(thresh(s, tau))
    u = r_(s - z)
    frac = []
    for _ in range(K):
        z_prev, u_prev = z, u
        v = r_(hty + r_(rho * r_(o.Dt_op(r_(z - u)))))
        x = r_(o._irfft12(np.asarray(C * np.asarray(o._rfft12(v), cdt), cdt), M, N))
        Dx = r_(o.D_op(x))
        s = r_(Dx + u)
        z = r_(thresh(s, tau))
        u = r_(s - z)
        frac.append(float(np.count_nonzero(z)) / z.size)
    f64 = lambda a: np.asarray(a, np.float64)   # noqa: E731  -- the norms themselves in fp64
    rr = _plane_norms(f64(Dx) - f64(z), 2)
    dd = float(rho) * _plane_norms(o.Dt_op(f64(z) - f64(z_prev)), 1)
    pri = np.maximum(_plane_norms(Dx, 2), _plane_norms(z, 2))
    dual = float(rho) * _plane_norms(o.Dt_op(f64(u)), 1)
    return {"x": o.to_c(f64(x).transpose(0, 1, 3, 2)), "state": state_to_c(f64(s)),
            "resid": np.stack([rr, dd, pri, dual], axis=-1), "r_alt": _plane_norms(f64(u) - f64(u_prev), 2),
            "prox_active": frac}


def prox_fraction(res):
    return float(np.mean(res["prox_active"]))


def stop_met(resid, M, N, eps_abs, eps_rel):
    """The stopping rule on every plane: |r| <= sqrt(2MN) eps_abs + eps_rel pri and |d| <= sqrt(MN) eps_abs + eps_rel dual."""
    r = np.asarray(resid, np.float64)
    return bool(np.all((r[..., 0] <= np.sqrt(2.0 * M * N) * eps_abs + eps_rel * r[..., 2])
                       & (r[..., 1] <= np.sqrt(1.0 * M * N) * eps_abs + eps_rel * r[..., 3])))


def solve_tol(y, lam, rho, h=None, iso=False, maxit=100, eps_abs=0.0, eps_rel=1e-3, check_every=10):
    """tvd_fft_tol in fp64: blocks of check_every iterations until the rule holds on every plane.  Returns (result of
    the last block, iterations run, the residuals of every block)."""
    state, it, hist, res = None, 0, [], None
    N, M = np.asarray(y).shape[-2:]
    while it < maxit:
        k = min(check_every, maxit - it)
        res = solve(y, lam, rho, h, iso, k, state)
        state = res["state"]
        it += k
        hist.append(res["resid"])
        if stop_met(res["resid"], M, N, eps_abs, eps_rel):
            break
    return res, it, hist
