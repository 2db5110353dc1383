"""Differentiable fp64 oracle of the grouped solve -- TEST INFRASTRUCTURE ONLY (a helper, not a test).

The torch restatement of tests/grouped_oracle.py (the loop of ops.jl:84-92 with C, H^T y, rho and tau held per plane),
built from oracle_torch's own pieces (_ht, _make_C), so that torch.autograd gives the gradient oracle of the grouped
adjoint (include/admm_deconv.h, admm_tvd_backward_grouped_dev_f32): y_bar per plane, h_bar per group's PSF, lambda_bar /
rho_bar per (lambda, rho) entry -- one entry shared by several groups collects the sum over them, as autograd does for
any shared leaf.  The isotropic prox keeps the reference's coupling: the pixel norm over every plane of the call.

Arrays are C layout (B, P, N, M) like the C ABI; PSFs are (kw, kh), stacked in group order g = b' * gp + p'."""
import numpy as np
import torch

from oracle_torch import _ht, _make_C


def group_of(b, p, gb, gp):
    return (b if gb > 1 else 0) * gp + (p if gp > 1 else 0)


def tvd_fft_grouped_torch(y, lam, rho, hs, gb, gp, isotropic=False, maxit=100, stats=None):
    """y: (B, P, N, M) tensor; lam, rho: tensors of 1 or gb * gp elements; hs: (G, kw, kh) tensor or None.
    stats (optional dict): 'prox_active' = per iteration the fraction of non-zero prox outputs, as oracle_np records."""
    B, P, N, M = y.shape
    G = gb * gp
    lam, rho = lam.reshape(-1), rho.reshape(-1)
    assert lam.numel() in (1, G) and rho.numel() in (1, G) and (hs is None or hs.shape[0] == G)
    assert not isotropic or (lam.numel() == 1 and rho.numel() == 1), "isotropic: one (lambda, rho) pair"
    pick = lambda v, g: v[g if v.numel() > 1 else 0]   # noqa: E731
    Cg = [_make_C(M, N, pick(rho, g), None if hs is None else hs[g]) for g in range(G)]
    gidx = [[group_of(b, p, gb, gp) for p in range(P)] for b in range(B)]
    C = torch.stack([torch.stack([Cg[gidx[b][p]] for p in range(P)]) for b in range(B)])
    hty = y if hs is None else torch.stack([torch.stack([_ht(y[b, p], hs[gidx[b][p]]) for p in range(P)])
                                            for b in range(B)])
    rho_p = torch.stack([torch.stack([pick(rho, gidx[b][p]) for p in range(P)]) for b in range(B)])[:, :, None, None]
    lam_p = torch.stack([torch.stack([pick(lam, gidx[b][p]) for p in range(P)]) for b in range(B)])[:, :, None, None]
    tau = lam_p / rho_p                                                  # ops.jl:20, per plane
    x = torch.zeros_like(y)
    z1 = torch.zeros_like(y); z2 = torch.zeros_like(y)
    u1 = torch.zeros_like(y); u2 = torch.zeros_like(y)
    for it in range(maxit):
        w1, w2 = z1 - u1, z2 - u2
        dtw = (w1 - torch.roll(w1, -1, dims=-2)) + (w2 - torch.roll(w2, -1, dims=-1))
        x = torch.fft.irfft2(C * torch.fft.rfft2(hty + rho_p * dtw), s=(N, M))
        d1 = x - torch.roll(x, 1, dims=-2)
        d2 = x - torch.roll(x, 1, dims=-1)
        s1, s2 = d1 + u1, d2 + u2
        if isotropic:
            nrm = torch.sqrt((s1 * s1 + s2 * s2).sum(dim=(0, 1), keepdim=True))   # every plane, whatever its group
            f = torch.clamp(1 - tau / nrm, min=0.0)
            z1, z2 = f * s1, f * s2
        else:
            z1 = torch.sign(s1) * torch.clamp(torch.abs(s1) - tau, min=0.0)
            z2 = torch.sign(s2) * torch.clamp(torch.abs(s2) - tau, min=0.0)
        if stats is not None and it < maxit - 1:
            nz = int(torch.count_nonzero(z1.detach())) + int(torch.count_nonzero(z2.detach()))
            stats.setdefault("prox_active", []).append(nz / (2 * z1.numel()))
        u1, u2 = u1 + d1 - z1, u2 + d2 - z2
    return x


def tvd_fft_grouped_grads(y, lam, rho, hs, gb, gp, iso, maxit, xbar, dtype=torch.float64, stats=None):
    """Autograd gradients of <xbar, x> in `dtype`: (x, y_bar, h_bar (G, kw, kh) or None, lam_bar (nparam,),
    rho_bar (nparam,)) as numpy arrays, nparam = the longer of lam and rho (a 1-element one is expanded first, as the
    library takes them, so its gradient comes back per group)."""
    yt = torch.as_tensor(np.asarray(y), dtype=dtype).clone().requires_grad_(True)
    lam = np.atleast_1d(np.asarray(lam, np.float64))
    rho = np.atleast_1d(np.asarray(rho, np.float64))
    n = max(lam.size, rho.size)
    lam_t = torch.tensor(np.broadcast_to(lam, (n,)).copy(), dtype=dtype, requires_grad=True)
    rho_t = torch.tensor(np.broadcast_to(rho, (n,)).copy(), dtype=dtype, requires_grad=True)
    h_t = None if hs is None else torch.as_tensor(np.stack(hs), dtype=dtype).clone().requires_grad_(True)
    x = tvd_fft_grouped_torch(yt, lam_t, rho_t, h_t, gb, gp, iso, maxit, stats)
    (x * torch.as_tensor(np.asarray(xbar), dtype=dtype)).sum().backward()
    g = lambda t: np.zeros(t.shape) if t.grad is None else t.grad.numpy()   # noqa: E731
    return x.detach().numpy(), g(yt), None if h_t is None else g(h_t), g(lam_t), g(rho_t)
