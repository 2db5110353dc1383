"""`tvd_fft` -- host-side mirror of the reference operator
`tvd_fft(y, λ, ρ, h, isotropic=false, maxit=100)` (/root/reference/src/ops/ops.jl:181-188).

The reference dispatches on the array type (`typeof(y) <: CuArray` -> tvd_fft_gpu, ops.jl:183);
here the device array is a torch tensor on a ROCm device and the body is the HIP library behind
the C ABI (include/admm_deconv.h).  Host (CPU) tensors are rejected: this package has no CPU
path (the CPU restatement under oracle/ is test infrastructure only).

Layout: a torch tensor of shape (B, P, N, M), C-contiguous float32, is byte-identical to the
reference's Julia array (M, N, P, B).  The PSF h is torch (kw, kh) == Julia (kh, kw).
"""
from __future__ import annotations

import contextlib
import ctypes
import math

import torch

from . import _lib

__all__ = ["tvd_fft", "tvd_fft_backward", "tvd_fft_record", "tvd_fft_backward_recorded", "Recording", "Workspace",
           "tvd_fft_multi", "tvd_fft_multi_backward_recorded", "multi_supported", "tvd_fft_grouped",
           "tvd_fft_grouped_record", "tvd_fft_grouped_backward_recorded", "tvd_fft_grouped_backward", "tvd_fft_grouped_grad",
           "GroupedRecording", "tvd_fft_state", "tvd_fft_tol"]


class Workspace:
    """Caller-owned device scratch for the solve (the library allocates nothing).

    A workspace serves one stream at a time: the solve's scratch state (C table, H^T y, s, spectra)
    lives in it for the whole enqueued solve.  `get(nbytes, device, stream)` marks the buffer as used on
    `stream`, so that a reallocation (or dropping the workspace) does not hand the memory to other work
    before that stream has finished with it."""

    def __init__(self):
        self._buf = None

    def get(self, nbytes, device, stream=None):
        # + 256: room for the 256-B alignment of the returned pointer
        if self._buf is None or self._buf.numel() < nbytes + 256 or self._buf.device != device:
            self._buf = torch.empty(max(nbytes, 256) + 256, dtype=torch.uint8, device=device)
        _record_streams(stream, device, self._buf)
        ptr = self._buf.data_ptr()
        off = (-ptr) % 256
        return ptr + off, self._buf.numel() - off


def _record_streams(stream, device, *tensors):
    """Mark tensors as used on `stream` when it is a torch stream other than the current one (the caching allocator
    must not hand their memory on before that stream is done).  The only place that compares streams."""
    if isinstance(stream, torch.cuda.Stream) and stream != torch.cuda.current_stream(device):
        for t in tensors:
            if t is not None:
                t.record_stream(stream)


# default workspaces, one per (kind, device, stream): concurrent solves on different streams (e.g. the
# branches of layers.Parallel) must not share scratch state
_default_ws = {}


def _default_workspace(kind, device, stream):
    return _default_ws.setdefault((kind, device, _stream_handle(stream)), Workspace())


def _stream_handle(stream):
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)


def _acquire(kind, nbytes, device, stream, workspace=None):
    """(workspace, pointer, length) of nbytes of scratch on `stream`: the caller's workspace (a recording's own), or
    the default one of this kind of call."""
    if workspace is None:
        workspace = _default_workspace(kind, device, stream)
    return (workspace, *workspace.get(nbytes, device, stream))


def _make_reducer(workspace, group):
    """admm_batch_reducer for a batch sharded over `group` (isotropic prox; include/admm_deconv.h).

    The library hands over a device pointer into `workspace` holding this shard's M x N partial map;
    the callback all-reduces (sum) that slice of the workspace tensor in place, on the library's
    stream.  gloo (CPU-only collectives) goes through a host copy.  Returns (struct, keep-alive)."""
    import torch.distributed as dist

    def cb(buf, count, stream, _user):
        try:
            base = workspace._buf.data_ptr()
            off = int(buf) - base
            view = workspace._buf[off: off + 4 * int(count)].view(torch.float32)
            ctx, lib_stream = contextlib.nullcontext(), None
            if view.is_cuda:
                # the stream the library enqueued the map on: handle 0 is torch's own default stream object (an
                # ExternalStream wrapped around handle 0 did not order torch's copies after the library's kernels:
                # a second sharded call read the map early, tests/test_gpu_dist_iso.py, round 6)
                h = int(stream or 0)
                cur = torch.cuda.current_stream(view.device)
                lib_stream = (cur if cur.cuda_stream == h else torch.cuda.default_stream(view.device) if h == 0
                              else torch.cuda.ExternalStream(h, device=view.device))
                ctx = torch.cuda.stream(lib_stream)
            with ctx:
                if dist.get_backend(group) == "gloo":
                    # host round trip (test infrastructure: gloo carries CPU tensors); the library launches its next
                    # kernel as soon as this returns, so the copy back must have landed by then
                    host = view.cpu()
                    dist.all_reduce(host, group=group)
                    view.copy_(host)
                    if lib_stream is not None:
                        lib_stream.synchronize()
                else:
                    dist.all_reduce(view, group=group)   # enqueued behind the library's work on its stream
            return 0
        except BaseException as e:   # an exception must not unwind through the C frames
            import sys
            print(f"admm_deconv batch reducer failed: {e!r}", file=sys.stderr)
            return -1

    fn = _lib.REDUCE_FN(cb)
    return _lib.BatchReducer(fn, None), fn


def _iso_arg(isotropic):
    """`isotropic` as the entry points carry it on: "plane" or a bool (one mapping to the C code, _lib.iso_code)."""
    return "plane" if _lib.iso_code(isotropic) == _lib.ISO_PLANE else bool(isotropic)


def _sharded(isotropic, group):
    # only the batch-coupled prox crosses shards (anisotropic and "plane": planes are independent, group is ignored)
    if group is None or _lib.iso_code(isotropic) != _lib.ISO_BATCH:
        return False
    import torch.distributed as dist
    return dist.is_initialized() and dist.get_world_size(group) > 1


class _DevScalars:
    """lambda / rho as device fp32 1-element tensors (the reference's `λ::CGPUArray`, ops.jl:99,181): the
    library reads them in-kernel, so the call needs no device-to-host read.  Holds the (possibly
    converted) tensors alive; `ptrs` are their device addresses."""

    __slots__ = ("lam", "rho")

    def __init__(self, lam, rho, device, stream):
        self.lam = self._one(lam, "lambda", device)
        self.rho = self._one(rho, "rho", device)
        _record_streams(stream, device, self.lam, self.rho)

    @staticmethod
    def _one(v, name, device):
        if isinstance(v, torch.Tensor):
            if v.numel() != 1:
                raise ValueError(f"{name} must have exactly one element (reference uses 1-element vectors)")
            t = v.detach().reshape(1)
            if t.device != device:
                if t.device.type == "cuda":
                    raise ValueError(f"{name} is on {t.device}, the solve on {device}")
                t = t.to(device)            # host tensor: one (blocking) upload
            return t.to(torch.float32).contiguous()
        # a host number next to a device tensor: a fill on the device, no transfer
        return torch.full((1,), _scalar(v, name), dtype=torch.float32, device=device)

    @property
    def ptrs(self):
        return self.lam.data_ptr(), self.rho.data_ptr()


def _on_device(lam, rho):
    return any(isinstance(v, torch.Tensor) and v.device.type == "cuda" for v in (lam, rho))


def _scalar(v, name):
    if isinstance(v, torch.Tensor):
        if v.numel() != 1:
            raise ValueError(f"{name} must have exactly one element (reference uses 1-element vectors)")
        v = v.detach().reshape(-1)[0].item()
    elif hasattr(v, "__len__"):
        if len(v) != 1:
            raise ValueError(f"{name} must have exactly one element")
        v = v[0]
    v = float(v)
    if not math.isfinite(v):
        raise ValueError(f"{name} must be finite")
    return v


def _stream_of(stream, device):
    if stream is None:
        stream = torch.cuda.current_stream(device)
    return stream, _stream_handle(stream)


def _forward_raw(y, lam, rho=1.0, h=None, isotropic=False, maxit=100, *, out=None, workspace=None, stream=None,
                 group=None):
    """ADMM TV deconvolution of every (M x N) plane of y (ops.jl:181).

    y:    torch float32 tensor (B, P, N, M) on a ROCm device (Julia (M,N,P,B)); a 2-D (N, M) or
          3-D (P, N, M) tensor is treated as B = 1 (and P = 1).
    lam, rho: host scalars, or 1-element tensors (the reference's 1-element vectors; default ρ = [1]).
          Device tensors are read in-kernel (admm_tvd_forward_dev_f32): no host synchronisation.
    h:    PSF tensor (kw, kh) (Julia (kh,kw,1,1)), or None / empty for the reference's empty PSF.
    Returns a new tensor x of y's shape (y is not modified)."""
    shape, y4, hbuf = _prep(y, h, ranks=(2, 3, 4))
    B, P, N, M = y4.shape
    kw, kh = (0, 0) if hbuf is None else hbuf.shape
    hp = None if hbuf is None else hbuf.data_ptr()
    out = _out_like(out, y4)
    stream, s_handle = _stream_of(stream, y.device)
    workspace, ws_ptr, ws_len = _acquire("fwd", _lib.workspace_bytes(M, N, P, B, kh, kw, isotropic), y.device, stream,
                                         workspace)
    red, keep = _make_reducer(workspace, group) if _sharded(isotropic, group) else (None, None)
    if _on_device(lam, rho):
        dv = _DevScalars(lam, rho, y.device, stream)
        _lib.check(_lib.load().admm_tvd_forward_dev_f32(
            y4.data_ptr(), out.data_ptr(), M, N, P, B, hp, kh, kw, *dv.ptrs, _lib.iso_code(isotropic), int(maxit),
            ws_ptr, ws_len, s_handle, ctypes.byref(red) if red is not None else None))
    elif red is not None:
        _lib.check(_lib.load().admm_tvd_forward_sharded_f32(
            y4.data_ptr(), out.data_ptr(), M, N, P, B, hp, kh, kw, _scalar(lam, "lambda"), _scalar(rho, "rho"), 1,
            int(maxit), ws_ptr, ws_len, s_handle, ctypes.byref(red)))
    else:
        _lib.check(_lib.load().admm_tvd_forward_f32(
            y4.data_ptr(), out.data_ptr(), M, N, P, B, hp, kh, kw, _scalar(lam, "lambda"), _scalar(rho, "rho"),
            _lib.iso_code(isotropic), int(maxit), ws_ptr, ws_len, s_handle))
    del keep
    return out.reshape(shape)


def _check_y(y, who, ranks=None, ranks_text=""):
    """y of every entry point: a float32 tensor on a ROCm device (the reference's T; this package has no CPU path),
    of one of the given ranks."""
    if not isinstance(y, torch.Tensor) or y.device.type != "cuda" or y.dtype != torch.float32:
        raise TypeError(f"{who}: y must be a float32 torch tensor on a ROCm device (no CPU path in this package)")
    if ranks is not None and y.dim() not in ranks:
        raise ValueError(f"{who}: y must be {ranks_text}")


def _out_like(out, y4):
    """The caller's output tensor, checked, or a new one."""
    if out is None:
        return torch.empty_like(y4)
    if out.shape != y4.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != y4.device:
        raise ValueError("out must be a contiguous float32 tensor of y's shape on y's device")
    return out


def _prep(y, h, ranks=None):
    """(y's shape, y as contiguous (B, P, N, M), the PSF as a contiguous float32 (kw, kh) on y's device or None)."""
    _check_y(y, "tvd_fft", ranks, "2-D, 3-D or 4-D")
    shape = y.shape
    y4 = y.reshape((1,) * (4 - y.dim()) + tuple(shape)).contiguous() if y.dim() < 4 else y.contiguous()
    if h is None or h.numel() == 0:
        return shape, y4, None
    hb = h.detach()
    while hb.dim() > 2 and hb.shape[0] == 1:
        hb = hb[0]
    if hb.dim() != 2:
        raise ValueError("PSF must be 2-D (kw, kh)")
    return shape, y4, hb.to(device=y.device, dtype=torch.float32).contiguous()


def _scalars_for(lam, rho, device, stream):
    """(device holder or None, host lambda, host rho): device tensors stay on the device."""
    if _on_device(lam, rho):
        return _DevScalars(lam, rho, device, stream), None, None
    return None, _scalar(lam, "lambda"), _scalar(rho, "rho")


def tvd_fft_backward(y, x_bar, lam, rho=1.0, h=None, isotropic=False, maxit=100, *, need_h=True, need_y=True,
                     need_rho=True, workspace=None, stream=None, group=None):
    """Adjoint of tvd_fft through all `maxit` unrolled iterations (what Zygote computes for the
    reference, src/train.jl:51).  Returns (x, y_bar, h_bar, lam_bar, rho_bar); h_bar is None without a PSF
    or when need_h is False; y_bar is None when need_y is False (the sweep then keeps no running sum of
    vbar unless h_bar needs it: 8 B/px less traffic per reverse step); rho_bar is None when need_rho is
    False (the fused and isotropic sweeps then skip s_k, which only rho_bar reads).  Recomputes the forward
    (x is returned for convenience).
    With `group` (isotropic prox, batch sharded over the group's ranks) h_bar / lam_bar / rho_bar are
    this shard's contributions: their sum over ranks is the gradient of the whole batch."""
    shape, y4, hb = _prep(y, h)
    B, P, N, M = y4.shape
    xb = x_bar.reshape(y4.shape).to(torch.float32).contiguous()
    kw, kh = (0, 0) if hb is None else hb.shape
    want_h = need_h and hb is not None
    stream, s_handle = _stream_of(stream, y.device)
    dv, lam_h, rho_h = _scalars_for(lam, rho, y.device, stream)
    nbytes = _lib.backward_workspace_bytes(M, N, P, B, kh, kw, isotropic, maxit, want_h)
    workspace, ws_ptr, ws_len = _acquire("bwd", nbytes, y.device, stream, workspace)
    x = torch.empty_like(y4)
    y_bar = torch.empty_like(y4) if need_y else None
    h_bar = torch.empty_like(hb) if want_h else None
    scal = torch.zeros(2, dtype=torch.float32, device=y.device)
    head = (y4.data_ptr(), xb.data_ptr(), y_bar.data_ptr() if need_y else None, h_bar.data_ptr() if want_h else None, scal.data_ptr(),
            scal.data_ptr() + 4 if need_rho else None, M, N, P, B, None if hb is None else hb.data_ptr(), kh, kw)
    tail = (_lib.iso_code(isotropic), int(maxit), x.data_ptr(), ws_ptr, ws_len, s_handle)
    red, keep = _make_reducer(workspace, group) if _sharded(isotropic, group) else (None, None)
    L = _lib.load()
    if dv is not None:
        _lib.check(L.admm_tvd_backward_dev_f32(*head, *dv.ptrs, *tail, ctypes.byref(red) if red is not None else None))
    elif red is not None:
        _lib.check(L.admm_tvd_backward_sharded_f32(*head, lam_h, rho_h, *tail, ctypes.byref(red)))
    else:
        _lib.check(L.admm_tvd_backward_f32(*head, lam_h, rho_h, *tail))
    del keep
    return x.reshape(shape), y_bar.reshape(shape) if need_y else None, h_bar, scal[0], scal[1] if need_rho else None


class Recording:
    """One forward solve recorded for its adjoint (admm_tvd_forward_record_f32): the trajectory lives in
    its own workspace until tvd_fft_backward_recorded consumes it, so a training step runs the forward
    once (no recompute in the backward).  Memory: about 8 B/px per iteration (plus 8 B/px of dim-2
    spectra per iteration with a PSF when h_bar is needed) -- sized for MI355X's 288 GB HBM."""

    __slots__ = ("workspace", "y4", "hb", "shape", "dv", "lam", "rho", "iso", "maxit", "want_h", "group", "dims",
                 "flags")


def tvd_fft_record(y, lam, rho=1.0, h=None, isotropic=False, maxit=100, *, need_h=True, need_rho=True, stream=None,
                   group=None):
    """Forward solve that records its trajectory.  Returns (x, Recording); see tvd_fft_backward_recorded.
    lam / rho as device tensors are read in-kernel (no host sync), as in tvd_fft.  need_rho=False: the
    replay will not be asked for rho_bar, so the fused 256 x 256 anisotropic path records only the
    soft-threshold branch of every trajectory element (ADMM_REC_MASKS: 16x less memory, a cheaper reverse
    sweep, the other gradients bitwise the same)."""
    shape, y4, hb = _prep(y, h)
    B, P, N, M = y4.shape
    stream, s_handle = _stream_of(stream, y.device)
    rec = Recording()
    rec.dv, rec.lam, rec.rho = _scalars_for(lam, rho, y.device, stream)
    kw, kh = (0, 0) if hb is None else hb.shape
    rec.want_h = bool(need_h and hb is not None)
    rec.y4, rec.hb, rec.shape, rec.iso, rec.maxit, rec.group = y4, hb, shape, _iso_arg(isotropic), int(maxit), group
    rec.dims = (M, N, P, B, kh, kw)
    rec.flags = (_lib.REC_HBAR if rec.want_h else 0) | (0 if need_rho else _lib.REC_MASKS)
    nbytes = _lib.backward_workspace_bytes(M, N, P, B, kh, kw, isotropic, maxit, rec.flags)
    rec.workspace, ws_ptr, ws_len = _acquire(None, nbytes, y.device, stream, Workspace())
    x = torch.empty_like(y4)
    red, keep = _make_reducer(rec.workspace, group) if _sharded(isotropic, group) else (None, None)
    head = (y4.data_ptr(), x.data_ptr(), M, N, P, B, None if hb is None else hb.data_ptr(), kh, kw)
    tail = (_lib.iso_code(rec.iso), rec.maxit, rec.flags, ws_ptr, ws_len, s_handle,
            ctypes.byref(red) if red is not None else None)
    L = _lib.load()
    if rec.dv is not None:
        _lib.check(L.admm_tvd_forward_record_dev_f32(*head, *rec.dv.ptrs, *tail))
    else:
        _lib.check(L.admm_tvd_forward_record_f32(*head, rec.lam, rec.rho, *tail))
    del keep
    return x.reshape(shape), rec


def tvd_fft_backward_recorded(rec, x, x_bar, *, stream=None, need_y=True, need_rho=True):
    """Reverse sweep of a recorded forward (x = that forward's output, unmodified).  Returns
    (y_bar, h_bar, lam_bar, rho_bar); h_bar is None unless the forward was recorded with need_h, y_bar is
    None when need_y is False (cheaper: no running sum of vbar unless h_bar needs it), rho_bar is None when
    need_rho is False (cheaper: the fused and isotropic sweeps then skip s_k, read for rho_bar only).
    Consumes the recording (its workspace is released)."""
    if rec.workspace is None:
        raise RuntimeError("recording already consumed")
    M, N, P, B, kh, kw = rec.dims
    y4, hb = rec.y4, rec.hb
    xb = x_bar.reshape(y4.shape).to(torch.float32).contiguous()
    x4 = x.reshape(y4.shape)
    if not x4.is_contiguous():
        raise ValueError("x must be the recorded forward's (contiguous) output")
    stream, s_handle = _stream_of(stream, y4.device)
    ws, ws_ptr, ws_len = _acquire(None, 0, y4.device, stream, rec.workspace)
    y_bar = torch.empty_like(y4) if need_y else None
    h_bar = torch.empty_like(hb) if rec.want_h else None
    scal = torch.zeros(2, dtype=torch.float32, device=y4.device)
    red, keep = _make_reducer(ws, rec.group) if _sharded(rec.iso, rec.group) else (None, None)
    head = (y4.data_ptr(), xb.data_ptr(), y_bar.data_ptr() if need_y else None, h_bar.data_ptr() if rec.want_h else None, scal.data_ptr(),
            scal.data_ptr() + 4 if need_rho else None, M, N, P, B, None if hb is None else hb.data_ptr(), kh, kw)
    tail = (_lib.iso_code(rec.iso), rec.maxit, x4.data_ptr(), ws_ptr, ws_len, s_handle,
            ctypes.byref(red) if red is not None else None)
    L = _lib.load()
    if rec.dv is not None:
        _record_streams(stream, y4.device, rec.dv.lam, rec.dv.rho)
        _lib.check(L.admm_tvd_backward_recorded_dev_f32(*head, *rec.dv.ptrs, *tail))
    else:
        _lib.check(L.admm_tvd_backward_recorded_f32(*head, rec.lam, rec.rho, *tail))
    del keep
    rec.workspace = None    # released once the stream has consumed it (caching allocator is stream-ordered)
    return y_bar.reshape(rec.shape) if need_y else None, h_bar, scal[0], scal[1] if need_rho else None


class _TvdFFTFn(torch.autograd.Function):
    """Differentiable tvd_fft: forward through the HIP solve, backward through the HIP adjoint
    (the rrule the Julia shim would register, julia/ADMMDeconvHIP.jl)."""

    @staticmethod
    def forward(ctx, y, lam_t, rho_t, h_t, isotropic, maxit, group, scalars):
        # the forward records its trajectory; the backward runs only the reverse sweep from it.  lam_t / rho_t
        # (device tensors) are read in-kernel unless the caller handed their host values in `scalars`
        need_h = h_t.numel() > 0 and ctx.needs_input_grad[3]
        lam, rho = scalars if scalars is not None else (lam_t, rho_t)
        # rho not trainable here (ADMMDeconvF2, F3): the recording keeps only the ST branches when it can
        x, ctx.rec = tvd_fft_record(y, lam, rho, h_t if h_t.numel() else None, isotropic, maxit,
                                    need_h=need_h, need_rho=ctx.needs_input_grad[2], group=group)
        # y (read again by the reverse sweep's h_bar correlation) and x are version-checked: an in-place
        # change of either between forward and backward raises instead of giving a wrong gradient
        ctx.save_for_backward(y, lam_t, rho_t, h_t, x)
        return x

    @staticmethod
    def backward(ctx, x_bar):
        _y, lam_t, rho_t, h_t, x = ctx.saved_tensors
        need_h = ctx.rec.want_h
        # y_bar only when y needs it (a first-layer denoiser's input does not): the sweep then skips Vsum
        yb, hb, lb, rb = tvd_fft_backward_recorded(ctx.rec, x, x_bar, need_y=ctx.needs_input_grad[0],
                                                   need_rho=ctx.needs_input_grad[2])
        ctx.rec = None
        hg = None
        if need_h:
            hg = hb.reshape(h_t.shape)
        return (yb if ctx.needs_input_grad[0] else None,
                lb.reshape(lam_t.shape).to(lam_t.dtype) if ctx.needs_input_grad[1] else None,
                rb.reshape(rho_t.shape).to(rho_t.dtype) if ctx.needs_input_grad[2] else None,
                hg, None, None, None, None)


def tvd_fft(y, lam, rho=1.0, h=None, isotropic=False, maxit=100, *, out=None, workspace=None, stream=None,
            group=None, scalars=None):
    """ADMM TV deconvolution of every (M x N) plane of y -- src/ops/ops.jl:181 semantics.

    y: float32 tensor (B,P,N,M) on a ROCm device (= Julia (M,N,P,B)); lam, rho: host scalars or
    1-element tensors -- device tensors (the reference's `λ::CGPUArray`) are read in-kernel, so the call
    never synchronises the host; h: PSF (kw,kh) (= Julia (kh,kw)) or None/empty.  Returns a new tensor.
    Differentiable (y, lam, rho, h) when autograd is recording and any of them requires grad
    (either prox); the gradient is the exact adjoint of the K unrolled iterations.
    group: torch.distributed group the batch is sharded over (each rank passes its own slice).  The
    isotropic prox's pixelnorm then spans the whole sharded batch (one M x N all-reduce per
    iteration), so every rank gets its slice of the unsharded result; ignored for the anisotropic
    prox and for isotropic="plane", whose planes are independent.
    isotropic: False (anisotropic TV), True (the reference's block-thresholding, whose pixel norm runs over every
    plane of the call: a plane's result depends on its batch) or "plane" (isotropic TV of each image plane on its
    own, sum over pixels of sqrt(dx^2 + dy^2): the result of a plane does not depend on the batch; 2-pass /
    runtime-length kernels; zero norm gives a zero factor, never NaN).
    scalars: optional host (lambda, rho) equal to the values of tensor lam / rho, used instead of the
    device values (gradients still flow to the tensors)."""
    tensors = [t for t in (y, lam, rho, h) if isinstance(t, torch.Tensor)]
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        dev = y.device
        as_t = lambda v: v if isinstance(v, torch.Tensor) else torch.full((1,), float(v), device=dev)  # noqa: E731
        h_t = h if isinstance(h, torch.Tensor) else torch.zeros(0, device=dev)
        return _TvdFFTFn.apply(y, as_t(lam), as_t(rho), h_t, _iso_arg(isotropic), int(maxit), group, scalars)
    if scalars is not None:
        lam, rho = scalars
    return _forward_raw(y, lam, rho, h, isotropic, maxit, out=out, workspace=workspace, stream=stream, group=group)


# ---- resumable solve: ADMM state in and out, residual norms, stop on tolerance (inference) ----
def tvd_fft_state(y, lam, rho=1.0, h=None, isotropic=False, maxit=100, *, state=None, want_state=True,
                  want_residuals=True, out=None, workspace=None, stream=None, _state_out=None):
    """`maxit` >= 1 ADMM iterations from the state `state` (None: the zero state, i.e. tvd_fft) -- returns (x, state,
    resid), each of the last two None where not wanted (admm_tvd_forward_state_dev_f32, include/admm_deconv.h).

    state: float32 (B, P, 2, N, M), s_k = D x_k + u_{k-1} (channel 0 the difference along N, channel 1 along M): all an
    ADMM solve carries over.  Feeding a call's state to the next continues the solve (a then b iterations = a + b);
    the call's own lam / rho form the prox of the given state, so a warm start under other parameters is well defined.
    resid: float32 (B, P, 4) = (|r|, |d|, pri, dual) per plane, the norms of the stopping rule (tvd_fft_tol).
    Neither `y` nor `state` is modified.  Not differentiable: ValueError when an input requires grad under autograd."""
    _lib.no_plane_mode(isotropic, "tvd_fft_state")
    tensors = [t for t in (y, lam, rho, h, state) if isinstance(t, torch.Tensor)]
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise ValueError("tvd_fft_state is not differentiable (use tvd_fft, or call it under torch.no_grad())")
    if int(maxit) < 1:
        raise ValueError("tvd_fft_state: maxit must be >= 1 (x is not part of the state)")
    _, y4, hbuf = _prep(y, h, ranks=(4,))
    B, P, N, M = y4.shape
    kw, kh = (0, 0) if hbuf is None else hbuf.shape
    if state is not None:
        if (not isinstance(state, torch.Tensor) or state.shape != (B, P, 2, N, M) or state.dtype != torch.float32
                or state.device != y.device):
            raise ValueError(f"state must be a float32 tensor of shape {(B, P, 2, N, M)} on y's device")
        state = state.detach().contiguous()
    out = _out_like(out, y4)
    stream, s_handle = _stream_of(stream, y.device)
    workspace, ws_ptr, ws_len = _acquire("state", _lib.state_workspace_bytes(M, N, P, B, kh, kw, isotropic), y.device,
                                         stream, workspace)
    dv = _DevScalars(lam, rho, y.device, stream)
    new = None
    if want_state:   # (_state_out: tvd_fft_tol's ping-pong tensor, of this shape by construction)
        new = _state_out if _state_out is not None else torch.empty((B, P, 2, N, M), dtype=torch.float32, device=y.device)
    resid = torch.empty((B, P, 4), dtype=torch.float32, device=y.device) if want_residuals else None
    _record_streams(stream, y.device, state, new, resid)
    _lib.check(_lib.load().admm_tvd_forward_state_dev_f32(
        y4.data_ptr(), out.data_ptr(), M, N, P, B, None if hbuf is None else hbuf.data_ptr(), kh, kw, *dv.ptrs,
        int(bool(isotropic)), int(maxit), None if state is None else state.data_ptr(),
        None if new is None else new.data_ptr(), None if resid is None else resid.data_ptr(), ws_ptr, ws_len, s_handle))
    return out, new, resid


def tvd_fft_tol(y, lam, rho=1.0, h=None, isotropic=False, maxit=100, *, eps_abs=0.0, eps_rel=1e-3, check_every=10,
                state=None, stream=None):
    """tvd_fft that stops on convergence: blocks of `check_every` iterations (the last one shorter, so that iters <=
    maxit) until every plane meets the standard ADMM stopping rule
        |r| <= sqrt(2 M N) eps_abs + eps_rel pri   and   |d| <= sqrt(M N) eps_abs + eps_rel dual
    (resid of tvd_fft_state).  Returns (x, state, iters, resid); iters is the total run.  The residuals are read back
    once per block -- the call's only host synchronisation.  `state`: an optional warm start."""
    _lib.no_plane_mode(isotropic, "tvd_fft_tol")
    maxit, check_every = int(maxit), int(check_every)
    if maxit < 1 or check_every < 1:
        raise ValueError("tvd_fft_tol: maxit and check_every must be >= 1")
    _check_y(y, "tvd_fft_tol", (4,), "4-D (B, P, N, M)")
    N, M = y.shape[-2:]
    a_pri, a_dual = math.sqrt(2.0 * M * N) * eps_abs, math.sqrt(1.0 * M * N) * eps_abs
    # lambda / rho once on the device: no per-block upload
    stream_t, _ = _stream_of(stream, y.device)
    dv = _DevScalars(lam, rho, y.device, stream_t)
    x = resid = None
    iters = 0
    spare = None   # two state tensors take turns: a block reads one and writes the other (never the caller's)
    while iters < maxit:
        k = min(check_every, maxit - iters)
        prev = state
        x, state, resid = tvd_fft_state(y, dv.lam, dv.rho, h, isotropic, k, state=prev, out=x, stream=stream,
                                        _state_out=spare)
        spare = prev if iters > 0 else None
        iters += k
        # the block's only synchronisation: the residuals, read back behind the solve on its stream
        with torch.cuda.stream(stream_t) if isinstance(stream_t, torch.cuda.Stream) else contextlib.nullcontext():
            if not isinstance(stream_t, torch.cuda.Stream):
                torch.cuda.synchronize(y.device)
            r = resid.to("cpu", torch.float64)
        if bool(((r[..., 0] <= a_pri + eps_rel * r[..., 2]) & (r[..., 1] <= a_dual + eps_rel * r[..., 3])).all()):
            break
    return x, state, iters, resid


# ---- several ADMM branches of one shared input (Parallel(chcat, ...), src/nets/net_build.jl:113-125) ----
MULTI_M = MULTI_N = 256


def _group_params(v, name, G, device):
    """lambda / rho of a grouped solve as a device float32 tensor of 1 or G elements (no host read)."""
    if isinstance(v, torch.Tensor):
        if v.numel() not in (1, G):
            raise ValueError(f"tvd_fft_grouped: {name} must have 1 or {G} (= gb * gp) elements, got {v.numel()}")
        t = v.detach().reshape(-1)
        if t.device != device:
            if t.device.type == "cuda":
                raise ValueError(f"{name} is on {t.device}, the solve on {device}")
            t = t.to(device)
        return t.to(torch.float32).contiguous()
    return torch.full((1,), _scalar(v, name), dtype=torch.float32, device=device)


def tvd_fft_grouped(y, lam, rho, h, isotropic=False, maxit=100, *, out=None, workspace=None, stream=None):
    """tvd_fft with a PSF, lambda and rho per image or per channel, in one call
    (admm_tvd_forward_grouped_dev_f32, include/admm_deconv.h).

    y:   float32 (B, P, N, M) on a ROCm device.
    h:   (gb, gp, kw, kh) with gb in {1, B} and gp in {1, P} -- plane (b, p) is solved with the PSF
         h[b if gb > 1 else 0, p if gp > 1 else 0] -- or None: no PSF; the groups then follow the parameter count
         (B * P values: per plane, B: per image, P: per channel, 1: one group; with B == P, B values name neither and
         are refused: give B * P).
    lam, rho: floats, or tensors of 1 or gb * gp elements (group order b * gp + p); they stay on the device.
    isotropic: True keeps the batch coupling of the reference over ALL planes, so lam and rho must have one element;
    "plane" (isotropic TV per plane) takes per-group lam and rho like the anisotropic prox.
    Not differentiable itself: tvd_fft_grouped_grad is the entry with the grouped adjoint."""
    _check_y(y, "tvd_fft_grouped", (4,), "4-D (B, P, N, M)")
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (y, h, lam, rho)):
        raise NotImplementedError("tvd_fft_grouped is the plain forward: call tvd_fft_grouped_grad for the grouped "
                                  "adjoint under autograd (or detach the inputs)")
    y4, hbuf, lt, rt, nparam, gb, gp = _grouped_args(y, lam, rho, h)
    B, P, N, M = y4.shape
    kw, kh = (0, 0) if hbuf is None else hbuf.shape[2:]
    hp = None if hbuf is None else hbuf.data_ptr()
    out = _out_like(out, y4)
    stream, s_handle = _stream_of(stream, y.device)
    nbytes = _lib.grouped_workspace_bytes(M, N, P, B, gb, gp, kh, kw, isotropic)
    workspace, ws_ptr, ws_len = _acquire("grouped", nbytes, y.device, stream, workspace)
    _record_streams(stream, y.device, lt, rt, hbuf)
    _lib.check(_lib.load().admm_tvd_forward_grouped_dev_f32(
        y4.data_ptr(), out.data_ptr(), M, N, P, B, gb, gp, hp, kh, kw, lt.data_ptr(), rt.data_ptr(), nparam,
        _lib.iso_code(isotropic), int(maxit), ws_ptr, ws_len, s_handle))
    return out


def _grouped_args(y, lam, rho, h):
    """A grouped call's arguments resolved: (y4, h (gb, gp, kw, kh) on the device or None, lambda and rho as device
    tensors of nparam elements each, nparam, gb, gp).  Nothing is read back to the host."""
    _check_y(y, "tvd_fft_grouped", (4,), "4-D (B, P, N, M)")
    y4 = y.detach().contiguous()
    B, P, N, M = y4.shape
    if h is None:
        gb = gp = 1
        hbuf, hp, kh, kw = None, None, 0, 0
        pg = [t.numel() for t in (lam, rho) if isinstance(t, torch.Tensor) and t.numel() > 1]
        if pg:   # no PSF: the groups come from the parameter count (per plane, per image or per channel)
            n = pg[0]
            if n == B * P:
                gb, gp = B, P
            elif n == B and n == P:
                raise ValueError(f"tvd_fft_grouped: {n} parameters without a PSF are ambiguous when B == P == {n} (per "
                                 "image or per channel?): give B * P values, one per plane in (b, p) order")
            elif n == B:
                gb = B
            elif n == P:
                gp = P
            else:
                raise ValueError(f"tvd_fft_grouped: {n} parameters fit neither B = {B}, P = {P} nor B * P planes")
    else:
        if not isinstance(h, torch.Tensor) or h.dim() != 4:
            raise ValueError("tvd_fft_grouped: h must be a 4-D tensor (gb, gp, kw, kh) or None")
        gb, gp, kw, kh = h.shape
        if gb not in (1, B) or gp not in (1, P):
            raise ValueError(f"tvd_fft_grouped: h's leading dims ({gb}, {gp}) must be (1 or B = {B}, 1 or P = {P})")
        hbuf = h.detach().to(device=y.device, dtype=torch.float32).contiguous()
    G = gb * gp
    lt, rt = _group_params(lam, "lambda", G, y.device), _group_params(rho, "rho", G, y.device)
    nparam = max(lt.numel(), rt.numel())
    if lt.numel() != nparam:
        lt = lt.expand(nparam).contiguous()
    if rt.numel() != nparam:
        rt = rt.expand(nparam).contiguous()
    return y4, hbuf, lt, rt, nparam, gb, gp


# ---- grouped adjoint (admm_tvd_backward_grouped_*, include/admm_deconv.h) ----
class GroupedRecording:
    """One grouped forward recorded for its adjoint (admm_tvd_forward_grouped_record_dev_f32); consumed by
    tvd_fft_grouped_backward_recorded.  Memory as Recording, plus one table set per group."""

    __slots__ = ("workspace", "y4", "hb", "lt", "rt", "nparam", "gb", "gp", "iso", "maxit", "want_h")


def _grouped_adjoint_args(y, lam, rho, h, isotropic, maxit, need_h):
    """A grouped adjoint call's arguments resolved (_grouped_args) into a GroupedRecording that holds no workspace yet."""
    _lib.no_plane_mode(isotropic, "the grouped adjoint")
    g = GroupedRecording()
    g.y4, g.hb, g.lt, g.rt, g.nparam, g.gb, g.gp = _grouped_args(y, lam, rho, h)
    g.iso, g.maxit, g.want_h, g.workspace = bool(isotropic), int(maxit), bool(need_h and g.hb is not None), None
    return g


def _grouped_geometry(g):
    """(M, N, P, B, gb, gp, h, kh, kw, lambda, rho, nparam, iso, maxit) as the C ABI's grouped entry points take them."""
    B, P, N, M = g.y4.shape
    kw, kh = (0, 0) if g.hb is None else g.hb.shape[2:]
    return (M, N, P, B, g.gb, g.gp, None if g.hb is None else g.hb.data_ptr(), kh, kw, g.lt.data_ptr(), g.rt.data_ptr(),
            g.nparam, int(g.iso), g.maxit)


def _grouped_workspace(g, kind, stream, workspace):
    geo = _grouped_geometry(g)
    nbytes = _lib.grouped_backward_workspace_bytes(*geo[:6], *geo[7:9], g.iso, g.maxit, _lib.REC_HBAR if g.want_h else 0)
    return _acquire(kind, nbytes, g.y4.device, stream, workspace)


def _grouped_sweep(fn, g, x, x_bar, ws, stream, need_y, need_rho):
    """The two adjoint entry points (recorded, combined): (y_bar, h_bar, lam_bar, rho_bar) of g through workspace ws."""
    y4 = g.y4
    xb = x_bar.reshape(y4.shape).to(torch.float32).contiguous()
    y_bar = torch.empty_like(y4) if need_y else None
    h_bar = torch.empty_like(g.hb) if g.want_h else None
    lam_bar = torch.zeros(g.nparam, dtype=torch.float32, device=y4.device)
    rho_bar = torch.zeros(g.nparam, dtype=torch.float32, device=y4.device) if need_rho else None
    outs = (y_bar, h_bar, lam_bar, rho_bar)
    _record_streams(stream, y4.device, g.lt, g.rt, g.hb)
    _lib.check(fn(y4.data_ptr(), xb.data_ptr(), *[None if t is None else t.data_ptr() for t in outs],
                  *_grouped_geometry(g), x.data_ptr(), *ws, _stream_handle(stream)))
    return outs


def tvd_fft_grouped_record(y, lam, rho, h, isotropic=False, maxit=100, *, need_h=True, stream=None):
    """tvd_fft_grouped that records its trajectory.  Returns (x, GroupedRecording).  need_h: the replay will be asked
    for h_bar (the dim-2 spectra are then recorded too, by the 2-pass forward)."""
    rec = _grouped_adjoint_args(y, lam, rho, h, isotropic, maxit, need_h)
    stream, s_handle = _stream_of(stream, y.device)
    rec.workspace, ws_ptr, ws_len = _grouped_workspace(rec, None, stream, Workspace())
    _record_streams(stream, y.device, rec.lt, rec.rt, rec.hb)
    x = torch.empty_like(rec.y4)
    _lib.check(_lib.load().admm_tvd_forward_grouped_record_dev_f32(
        rec.y4.data_ptr(), x.data_ptr(), *_grouped_geometry(rec), _lib.REC_HBAR if rec.want_h else 0, ws_ptr, ws_len,
        s_handle))
    return x, rec


def tvd_fft_grouped_backward_recorded(rec, x, x_bar, *, need_y=True, need_rho=True, stream=None):
    """Reverse sweep of a recorded grouped forward (x = that forward's output, unmodified).  Returns
    (y_bar, h_bar (gb, gp, kw, kh) or None, lam_bar (nparam,), rho_bar (nparam,) or None): one gradient per group's
    PSF; entry g of lam_bar / rho_bar sums over group g's planes (nparam = 1: over all planes).  Consumes the
    recording."""
    if rec.workspace is None:
        raise RuntimeError("recording already consumed")
    x4 = x.reshape(rec.y4.shape)
    if not x4.is_contiguous():
        raise ValueError("x must be the recorded forward's (contiguous) output")
    stream, _ = _stream_of(stream, rec.y4.device)
    ws = _acquire(None, 0, rec.y4.device, stream, rec.workspace)[1:]
    outs = _grouped_sweep(_lib.load().admm_tvd_backward_grouped_recorded_dev_f32, rec, x4, x_bar, ws, stream, need_y,
                          need_rho)
    rec.workspace = None
    return outs


def tvd_fft_grouped_backward(y, x_bar, lam, rho, h, isotropic=False, maxit=100, *, need_h=True, need_y=True,
                             need_rho=True, workspace=None, stream=None):
    """The grouped forward and its adjoint in one call.  Returns (x, y_bar, h_bar, lam_bar, rho_bar), shaped as
    tvd_fft_grouped_backward_recorded's."""
    g = _grouped_adjoint_args(y, lam, rho, h, isotropic, maxit, need_h)
    stream, _ = _stream_of(stream, y.device)
    ws = _grouped_workspace(g, "grouped_bwd", stream, workspace)[1:]
    x = torch.empty_like(g.y4)
    return (x, *_grouped_sweep(_lib.load().admm_tvd_backward_grouped_dev_f32, g, x, x_bar, ws, stream, need_y, need_rho))


class _TvdFFTGroupedFn(torch.autograd.Function):
    """Differentiable tvd_fft_grouped: one recorded grouped forward, one reverse sweep."""

    @staticmethod
    def forward(ctx, y, lam_t, rho_t, h_t, isotropic, maxit):
        has_h = h_t.numel() > 0
        x, ctx.rec = tvd_fft_grouped_record(y, lam_t, rho_t, h_t if has_h else None, isotropic, maxit,
                                            need_h=has_h and ctx.needs_input_grad[3])
        ctx.save_for_backward(y, lam_t, rho_t, h_t, x)
        return x

    @staticmethod
    def backward(ctx, x_bar):
        _y, lam_t, rho_t, h_t, x = ctx.saved_tensors
        need = ctx.needs_input_grad
        yb, hb, lb, rb = tvd_fft_grouped_backward_recorded(ctx.rec, x, x_bar, need_y=need[0], need_rho=need[2])
        ctx.rec = None

        def shaped(g, p):   # a 1-element parameter next to per-group ones gets the sum over the groups
            if g.numel() != p.numel():
                g = g.sum()
            return g.reshape(p.shape).to(p.dtype)
        return (yb if need[0] else None, shaped(lb, lam_t) if need[1] else None, shaped(rb, rho_t) if need[2] else None,
                hb.reshape(h_t.shape).to(h_t.dtype) if ctx.needs_input_grad[3] and hb is not None else None, None, None)


def tvd_fft_grouped_grad(y, lam, rho, h, isotropic=False, maxit=100):
    """tvd_fft_grouped under autograd: when y, h, lam or rho requires grad, one recorded grouped forward and one
    reverse sweep (the dim-2 spectra for h_bar are recorded only if h requires grad; rho_bar and y_bar are formed only
    if wanted).  Gradients come back in the shapes given: h.grad (gb, gp, kw, kh); a 1-element lam next to per-group
    rho gets the sum over the groups; a Python float gets none.  Without grad it is the plain call."""
    _lib.no_plane_mode(isotropic, "tvd_fft_grouped_grad")
    ts = [t for t in (y, lam, rho, h) if isinstance(t, torch.Tensor)]
    if not (torch.is_grad_enabled() and any(t.requires_grad for t in ts)):
        return tvd_fft_grouped(y, lam, rho, h, isotropic, maxit)
    dev = y.device
    as_t = lambda v: v if isinstance(v, torch.Tensor) else torch.full((1,), float(v), device=dev)  # noqa: E731
    h_t = h if h is not None else torch.empty(0, device=dev)
    return _TvdFFTGroupedFn.apply(y, as_t(lam), as_t(rho), h_t, bool(isotropic), int(maxit))


def multi_supported(y, isotropic=False, psf=None, group=None):
    """Whether the one-grid multi-branch solve (admm_tvd_forward_multi_dev_f32) covers this input: the fused
    256 x 256 kernels (anisotropic, or isotropic with the fused reverse sweep on; never isotropic="plane"), no PSF,
    one process holding the batch, and the fused option on."""
    return (_lib.iso_code(isotropic) != _lib.ISO_PLANE and isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.float32 and y.dim() == 4
            and y.shape[-1] == MULTI_M and y.shape[-2] == MULTI_N
            and (not isotropic or _lib.get_option("FUSED_ADJ") == 1)
            and (psf is None or psf.numel() == 0) and group is None and _lib.get_option("FUSED") == 1)


class MultiRecording:
    """A multi-branch forward recorded for its reverse sweep (tvd_fft_multi(record=True))."""
    __slots__ = ("workspace", "dims", "maxit", "masks", "dv")


def _ptr_array(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def tvd_fft_multi(y, lams, rhos, maxit=100, *, out=None, record=False, need_rho=True, isotropic=False, workspace=None,
                  stream=None):
    """x = chcat(tvd_fft(y, lams[0], rhos[0], nothing, false, maxit), ..., tvd_fft(y, lams[n-1], ...)) in ONE
    launch of the fused kernel (every branch's planes in one grid).  y: (B, P, 256, 256) float32 on the
    device; lams, rhos: n 1-element tensors / numbers (device tensors read in-kernel).  Returns x of shape
    (B, n * P, 256, 256) -- the chcat layout, branch i's channels at i*P..i*P+P-1 -- and, with record=True,
    a MultiRecording for tvd_fft_multi_backward_recorded (need_rho=False: only the ST branches are kept).
    isotropic=True: the BT prox (ops.jl:6,10), each branch's norm over its own planes; its recording never
    gives rho_bar (the fused isotropic sweep, plane_iso.hip)."""
    _lib.no_plane_mode(isotropic, "tvd_fft_multi")
    if not multi_supported(y, isotropic):
        raise ValueError("tvd_fft_multi: y must be a float32 (B, P, 256, 256) ROCm tensor (fused options on)")
    if record and isotropic and need_rho:
        raise ValueError("tvd_fft_multi: an isotropic recording gives lambda_bar and y_bar only (need_rho=False)")
    n = len(lams)
    if n < 1 or len(rhos) != n:
        raise ValueError("tvd_fft_multi: one lambda and one rho per branch")
    y4 = y.contiguous()
    B, P, N, M = y4.shape
    stream, s_handle = _stream_of(stream, y.device)
    dv = [_DevScalars(l, r, y.device, stream) for l, r in zip(lams, rhos)]
    flags = (_lib.MULTI_RECORD | (0 if need_rho else _lib.REC_MASKS)) if record else 0
    if isotropic:
        flags |= _lib.MULTI_ISO
    nbytes = _lib.multi_workspace_bytes(M, N, P, B, n, maxit, flags)
    workspace, ws_ptr, ws_len = _acquire("multi", nbytes, y.device, stream, Workspace() if record else workspace)
    if out is None:
        out = torch.empty((B, n * P, N, M), dtype=torch.float32, device=y.device)
    elif out.shape != (B, n * P, N, M) or not out.is_contiguous():
        raise ValueError("out must be a contiguous (B, n*P, N, M) float32 tensor")
    lp, rp = _ptr_array([d.lam for d in dv]), _ptr_array([d.rho for d in dv])
    _lib.check(_lib.load().admm_tvd_forward_multi_dev_f32(y4.data_ptr(), out.data_ptr(), M, N, P, B, n, lp, rp,
                                                          int(maxit), flags, ws_ptr, ws_len, s_handle))
    if not record:
        return out
    rec = MultiRecording()
    rec.workspace, rec.dims, rec.maxit, rec.masks, rec.dv = (workspace, (M, N, P, B, n), int(maxit),
                                                             not need_rho or isotropic, dv)
    return out, rec


def tvd_fft_multi_backward_recorded(rec, x, x_bar, *, need_y=True, need_rho=True, stream=None):
    """Reverse sweep of a recorded multi-branch forward (x = its output, unmodified; x_bar in x's chcat
    layout).  Returns (y_bar or None, lam_bar (n,), rho_bar (n,) or None); y_bar sums the branches' input
    gradients.  Consumes the recording."""
    if rec.workspace is None:
        raise RuntimeError("recording already consumed")
    M, N, P, B, n = rec.dims
    if need_rho and rec.masks:
        raise ValueError("recorded with need_rho=False: rho_bar is not available")
    stream, s_handle = _stream_of(stream, x.device)
    xb = x_bar.reshape(x.shape).to(torch.float32).contiguous()
    _, ws_ptr, ws_len = _acquire(None, 0, x.device, stream, rec.workspace)
    y_bar = torch.empty((B, P, N, M), dtype=torch.float32, device=x.device) if need_y else None
    scal = torch.zeros(2 * n, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().admm_tvd_backward_multi_recorded_dev_f32(
        xb.data_ptr(), y_bar.data_ptr() if need_y else None, scal.data_ptr(),
        scal.data_ptr() + 4 * n if need_rho else None, M, N, P, B, n, rec.maxit, x.data_ptr(), ws_ptr, ws_len,
        s_handle))
    rec.workspace = None
    return y_bar, scal[:n], scal[n:] if need_rho else None


class _TvdFFTMultiFn(torch.autograd.Function):
    """Differentiable tvd_fft_multi: one recorded forward of every branch, one reverse sweep."""

    @staticmethod
    def forward(ctx, y, maxit, iso, n, *params):
        lams, rhos = params[:n], params[n:]
        ctx.n = n
        need_rho = any(ctx.needs_input_grad[4 + n + i] for i in range(n))
        if iso and need_rho:
            raise NotImplementedError("rho_bar of the isotropic multi-branch solve: solve the branches one by one")
        x, ctx.rec = tvd_fft_multi(y, lams, rhos, maxit, record=True, need_rho=need_rho, isotropic=iso)
        ctx.need_rho = need_rho
        ctx.save_for_backward(y, x, *params)
        return x

    @staticmethod
    def backward(ctx, x_bar):
        y, x, *params = ctx.saved_tensors
        n = ctx.n
        yb, lb, rb = tvd_fft_multi_backward_recorded(ctx.rec, x, x_bar, need_y=ctx.needs_input_grad[0],
                                                     need_rho=ctx.need_rho)
        ctx.rec = None
        grads = [yb if ctx.needs_input_grad[0] else None, None, None, None]
        for i in range(n):
            p = params[i]
            grads.append(lb[i:i + 1].reshape(p.shape).to(p.dtype) if ctx.needs_input_grad[4 + i] else None)
        for i in range(n):
            p = params[n + i]
            grads.append(rb[i:i + 1].reshape(p.shape).to(p.dtype) if ctx.needs_input_grad[4 + n + i] else None)
        return tuple(grads)


def tvd_fft_multi_grad(y, lams, rhos, maxit=100, isotropic=False):
    """tvd_fft_multi under autograd when y or any lam / rho tensor requires grad (else the plain call)."""
    _lib.no_plane_mode(isotropic, "tvd_fft_multi_grad")
    ts = [t for t in (y, *lams, *rhos) if isinstance(t, torch.Tensor)]
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        dev = y.device
        as_t = lambda v: v if isinstance(v, torch.Tensor) else torch.full((1,), float(v), device=dev)  # noqa: E731
        return _TvdFFTMultiFn.apply(y, int(maxit), bool(isotropic), len(lams), *[as_t(v) for v in lams],
                                    *[as_t(v) for v in rhos])
    return tvd_fft_multi(y, lams, rhos, maxit, isotropic=isotropic)
