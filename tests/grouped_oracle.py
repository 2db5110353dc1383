"""fp64 oracle of the grouped solve (include/admm_deconv.h, admm_tvd_forward_grouped_dev_f32): the loop of
oracle_np.tvd_fft_literal (ops.jl:84-92) with C, H^T y, rho and tau held per plane, built from oracle_np's own pieces.

Plane (b, p) belongs to group g = (b if gb > 1 else 0) * gp + (p if gp > 1 else 0) and takes that group's PSF,
lambda and rho.  Anisotropic planes stay independent; the isotropic prox keeps the reference's coupling (pixelnorm over
every plane of the call, ops.jl:6) and therefore one (lambda, rho) pair."""
import numpy as np

from oracle_np import BT, ST, D_op, Dt_op, Ht_op, _irfft12, _record_prox, _rfft12, make_C


def group_of(b, p, gb, gp):
    return (b if gb > 1 else 0) * gp + (p if gp > 1 else 0)


def tvd_fft_grouped(y, lam, rho, hs, gb, gp, isotropic=False, maxit=100, stats=None):
    """y: (M, N, P, B) Julia-order array; hs: list of gb * gp PSFs (kh, kw) in group order, or None (no PSF);
    lam, rho: 1 or gb * gp values (rounded to fp32 by the caller as the library takes them).  Returns x (M, N, P, B)."""
    y = np.asarray(y, np.float64)
    M, N, P, B = y.shape
    G = gb * gp
    lam = np.broadcast_to(np.asarray(lam, np.float64).ravel(), (G,)) if np.size(lam) == 1 else np.asarray(lam, np.float64)
    rho = np.broadcast_to(np.asarray(rho, np.float64).ravel(), (G,)) if np.size(rho) == 1 else np.asarray(rho, np.float64)
    assert lam.shape == rho.shape == (G,) and (hs is None or len(hs) == G)
    assert not isotropic or (np.all(lam == lam[0]) and np.all(rho == rho[0])), "isotropic: one (lambda, rho) pair"
    yp = y.transpose(0, 1, 3, 2)                                   # (M, N, B, P), ops.jl:19
    C = np.empty((M // 2 + 1, N, B, P))
    hty = np.empty((M, N, B, P))
    rho_p = np.empty((1, 1, B, P))
    tau_p = np.empty((1, 1, B, P))
    for b in range(B):
        for p in range(P):
            g = group_of(b, p, gb, gp)
            h = None if hs is None else np.asarray(hs[g], np.float64)
            C[:, :, b, p] = make_C(M, N, rho[g], h)
            hty[:, :, b:b + 1, p:p + 1] = yp[:, :, b:b + 1, p:p + 1] if h is None else Ht_op(yp[:, :, b:b + 1, p:p + 1], h)
            rho_p[0, 0, b, p], tau_p[0, 0, b, p] = rho[g], lam[g] / rho[g]
    tau2 = np.repeat(tau_p, 2, axis=2)                             # both difference channels of image b
    thresh = BT if isotropic else ST
    z = np.zeros((M, N, 2 * B, P))
    u = np.zeros((M, N, 2 * B, P))
    x = np.zeros((M, N, B, P))
    for k in range(maxit):                                         # ops.jl:84-92
        x = _irfft12(C * _rfft12(hty + rho_p * Dt_op(z - u)), M, N)
        Dxk = D_op(x)
        z = thresh(Dxk + u, tau2)
        _record_prox(stats, z, maxit, k)
        u = u + Dxk - z
    return x.transpose(0, 1, 3, 2)
