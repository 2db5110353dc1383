"""Oracle helpers of the per-plane isotropic mode (isotropic="plane", ADMM_ISO_PLANE): isotropic TV of every image
plane on its own.  Nothing new under oracle/: the mode IS the reference's isotropic solve (ops.jl:6,10 through
tests/state_oracle.py / oracle/oracle_np.py) called on one (M, N, 1, 1) plane at a time, where pixelnorm runs over
that plane's two difference channels only.

  solve_loop     the definition: state_oracle.solve(y[b:b+1, p:p+1], ..., iso=True) per plane
  solve_direct   an independent form: one ADMM loop over the whole batch from oracle_np's operators with its own
                 block-thresholding over a (M, N, B, 2, P) view of the state (zero norm -> zero factor, as the library)
  grads_loop     per-plane gradients from oracle_torch.tvd_fft_grads: y_bar per plane, h_bar / lam_bar / rho_bar summed
  model_grads    tests/kernel_model.py tvd_model_grads(iso=True) one plane at a time, summed the same way
  margin         min over k and pixels of | |s_k| - tau | in the fp64 oracle: how far the adjoint case sits from the
                 kink of the prox, where an fp32 trajectory may take the other branch

Inputs are the length sweep's white noise: rng = default_rng(seed), y the first draw, x_bar the next."""
import numpy as np

import oracle_np as o
import state_oracle

LAM, RHO = 0.05, 0.1   # tau = 0.5


def gaussian_psf(k, sigma=1.0):
    """k x k Gaussian PSF (kw, kh), float32, unit sum; None for k = 0."""
    if k == 0:
        return None
    a = np.arange(k, dtype=np.float64) - (k - 1) / 2.0
    g = np.exp(-(a[:, None] ** 2 + a[None, :] ** 2) / (2.0 * sigma * sigma))
    return (g / g.sum()).astype(np.float32)


def inputs(B, P, N, M, k, seed):
    """(y, x_bar, h): y and x_bar float32 (B, P, N, M), in that order of draws; h the Gaussian PSF or None."""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((B, P, N, M)).astype(np.float32)
    xbar = rng.standard_normal((B, P, N, M)).astype(np.float32)
    return y, xbar, gaussian_psf(k)


def solve_loop(y, lam, rho, h, K, dtype=np.float64, stats=None):
    """x (B, P, N, M) float64: every plane solved alone by the isotropic oracle.  stats (dict): "nonzero" = the
    fraction of non-zero prox outputs z_k over all planes and iterations."""
    y = np.asarray(y)
    B, P = y.shape[:2]
    x = np.empty(y.shape, np.float64)
    frac = []
    for b in range(B):
        for p in range(P):
            r = state_oracle.solve(y[b:b + 1, p:p + 1], lam, rho, h, iso=True, K=K, dtype=dtype)
            x[b, p] = r["x"][0, 0]
            frac.append(state_oracle.prox_fraction(r))
    if stats is not None:
        stats["nonzero"] = float(np.mean(frac))
    return x


def _bt_plane(s, tau):
    """Block-thresholding of each pixel's own 2-vector: s (M, N, 2B, P), channels 2b and 2b + 1 of plane (b, p)."""
    M, N, B2, P = s.shape
    v = s.reshape(M, N, B2 // 2, 2, P)
    n = np.sqrt((v * v).sum(axis=3, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(n > tau, np.maximum(1.0 - tau / n, 0.0), 0.0)
    return (f * v).reshape(s.shape), n.reshape(M, N, B2 // 2, P)


def solve_direct(y, lam, rho, h, K, want_margin=False):
    """The same solve as one fp64 loop over the whole batch (ops.jl:84-92 from oracle_np's operators) with _bt_plane
    as the prox.  want_margin: also min over k = 1..K-1 and pixels of | |s_k| - tau | (the states the adjoint reads)."""
    yj = o.from_c(np.asarray(y, np.float64))
    M, N, P, B = yj.shape
    lam = np.float64(np.float32(lam))
    rho = np.float64(np.float32(rho))
    tau = lam / rho
    yp = yj.transpose(0, 1, 3, 2)
    hj = o.psf_from_c(h)
    hj = None if hj is None or np.size(hj) == 0 else np.asarray(hj, np.float64)
    C = o.make_C(M, N, float(rho), hj)[:, :, None, None]
    hty = yp.copy() if hj is None else o.Ht_op(yp, hj)
    z = np.zeros((M, N, 2 * B, P))
    u = np.zeros_like(z)
    margin = np.inf
    for k in range(1, K + 1):
        v = hty + rho * o.Dt_op(z - u)
        x = o._irfft12(C * o._rfft12(v), M, N)
        s = o.D_op(x) + u
        z, n = _bt_plane(s, tau)
        u = s - z
        if k < K:
            margin = min(margin, float(np.abs(n - tau).min()))
    xc = o.to_c(x.transpose(0, 1, 3, 2))
    return (xc, margin) if want_margin else xc


def margin(y, lam, rho, h, K):
    return solve_direct(y, lam, rho, h, K, want_margin=True)[1]


def _sum_grads(per_plane, y_shape, h):
    ybar = np.empty(y_shape, np.float64)
    hbar = None if h is None else np.zeros(np.asarray(h).shape, np.float64)
    lb = rb = 0.0
    for (b, p), (yb, hb, l, r) in per_plane.items():
        ybar[b, p] = yb
        if hbar is not None:
            hbar += hb
        lb += l
        rb += r
    return ybar, hbar, lb, rb


def grads_loop(y, lam, rho, h, K, xbar, dtype=None):
    """Gradients of sum over planes of <xbar, x>: (x, ybar (B, P, N, M), hbar (kw, kh) or None, lam_bar, rho_bar) from
    torch autograd of the isotropic oracle, one (1, 1, N, M) plane at a time (dtype: torch.float64 by default)."""
    import torch

    import oracle_torch
    dtype = torch.float64 if dtype is None else dtype
    y = np.asarray(y)
    B, P = y.shape[:2]
    x = np.empty(y.shape, np.float64)
    per = {}
    for b in range(B):
        for p in range(P):
            xs, yb, hb, l, r = oracle_torch.tvd_fft_grads(y[b:b + 1, p:p + 1], np.float32(lam), np.float32(rho), h, True, K,
                                                          xbar[b:b + 1, p:p + 1], dtype=dtype)
            x[b, p] = np.asarray(xs, np.float64)[0, 0]
            per[(b, p)] = (np.asarray(yb, np.float64)[0, 0], None if hb is None else np.asarray(hb, np.float64), l, r)
    return (x, *_sum_grads(per, y.shape, h))


def model_grads(y, lam, rho, h, K, xbar):
    """The kernels' reverse sweep restated (kernel_model.tvd_model_grads(iso=True)) on one plane at a time."""
    import kernel_model
    y = np.asarray(y)
    B, P = y.shape[:2]
    x = np.empty(y.shape, np.float64)
    per = {}
    lam64, rho64 = float(np.float32(lam)), float(np.float32(rho))
    for b in range(B):
        for p in range(P):
            xs, yb, hb, l, r = kernel_model.tvd_model_grads(y[b, p][None], lam64, rho64, h, K,
                                                            np.asarray(xbar[b, p][None], np.float64), iso=True)
            x[b, p] = xs[0]
            per[(b, p)] = (yb[0], hb, l, r)
    return (x, *_sum_grads(per, y.shape, h))


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def worst_plane_rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    a2, b2 = a.reshape(-1, a.shape[-2] * a.shape[-1]), b.reshape(-1, a.shape[-2] * a.shape[-1])
    return max(rel_l2(a2[i], b2[i]) for i in range(a2.shape[0]))
