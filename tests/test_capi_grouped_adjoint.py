"""CPU: the grouped adjoint's C ABI (include/admm_deconv.h) -- exports, workspace size, argument refusals, the
recordings registry's refusals and the path decision.  No GPU work is issued: every refusal comes before the first
launch."""
import ctypes
import os
import re

import pytest

from admm_deconv import _lib

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "admm_deconv.h")
NAMES = ("admm_tvd_grouped_backward_workspace_bytes", "admm_tvd_forward_grouped_record_dev_f32",
         "admm_tvd_backward_grouped_recorded_dev_f32", "admm_tvd_backward_grouped_dev_f32", "admm_query_grouped_paths")
FAKE = 1 << 20   # a "device pointer" that is never dereferenced: validation fails first


def test_header_binding_and_library_export_the_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    L = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert n in _lib.EXPORTS, n
        assert hasattr(L, n), n
    assert L.admm_abi_version() == 3   # symbols were added only


def test_workspace_covers_the_single_adjoint_and_grows():
    q = _lib.grouped_backward_workspace_bytes
    for (M, N, P, B, kh, iso) in ((256, 256, 2, 4, 15, False), (64, 32, 3, 2, 5, True), (63, 45, 3, 2, 5, False)):
        for flags in (0, _lib.REC_HBAR):
            assert q(M, N, P, B, 1, 1, kh, kh, iso, 6, flags) >= _lib.backward_workspace_bytes(M, N, P, B, kh, kh, iso, 6, flags)
    one = q(256, 256, 2, 4, 1, 1, 15, 15, False, 6)
    per_image = q(256, 256, 2, 4, 4, 1, 15, 15, False, 6)
    per_plane = q(256, 256, 2, 4, 4, 2, 15, 15, False, 6)
    assert one < per_image < per_plane                                          # with G
    assert per_plane < q(256, 256, 2, 4, 4, 2, 15, 15, False, 7)                 # with maxit (a trajectory slot)
    assert per_plane < q(256, 256, 2, 4, 4, 2, 15, 15, False, 6, _lib.REC_HBAR)  # with the h_bar trajectory
    # ADMM_REC_MASKS is accepted and not honoured: the full trajectory
    assert q(256, 256, 1, 128, 128, 1, 15, 15, False, 6, _lib.REC_MASKS) == q(256, 256, 1, 128, 128, 1, 15, 15, False, 6)
    assert q(8, 8, 1, 65280, 65280, 1, 3, 3, False, 2) > 0                       # the most planes of one call


@pytest.mark.parametrize("args,code", [
    ((64, 32, 3, 2, 3, 1, 5, 5, 0, 5, 0), _lib.ADMM_E_INVALID),        # gb neither 1 nor B
    ((64, 32, 3, 2, 1, 2, 5, 5, 0, 5, 0), _lib.ADMM_E_INVALID),        # gp neither 1 nor P
    ((64, 32, 3, 2, 0, 1, 5, 5, 0, 5, 0), _lib.ADMM_E_INVALID),
    ((64, 32, 3, 2, 2, 3, 5, 0, 0, 5, 0), _lib.ADMM_E_INVALID),        # half-empty PSF
    ((64, 32, 3, 2, 2, 3, 5, 5, 0, -1, 0), _lib.ADMM_E_INVALID),       # maxit
    ((8192, 32, 3, 2, 2, 3, 5, 5, 0, 5, 0), _lib.ADMM_E_UNSUPPORTED),  # shapes as check_shape
    ((64, 32, 3, 2, 2, 3, 65, 5, 0, 5, 0), _lib.ADMM_E_UNSUPPORTED),   # kh > M
    ((8, 8, 1, 65281, 1, 1, 3, 3, 0, 5, 0), _lib.ADMM_E_UNSUPPORTED),  # above 65,280 planes
])
def test_workspace_query_refusals(args, code):
    out = ctypes.c_size_t(0)
    L = _lib.load()
    assert L.admm_tvd_grouped_backward_workspace_bytes(*args, ctypes.byref(out)) == code
    assert len(L.admm_last_error()) > 0
    assert L.admm_tvd_grouped_backward_workspace_bytes(64, 32, 3, 2, 2, 3, 5, 5, 0, 5, 0, None) == _lib.ADMM_E_INVALID


def _geom(kw):
    d = dict(M=64, N=32, P=3, B=2, gb=2, gp=3, h=FAKE, kh=5, kw=5, lam=FAKE, rho=FAKE, nparam=6, iso=0, maxit=5, y=FAKE,
             x=FAKE, ws=FAKE, ws_bytes=1 << 40, x_bar=FAKE, y_bar=FAKE, h_bar=None, lam_bar=FAKE, rho_bar=FAKE, flags=0)
    d.update(kw)
    return d


def _record(**kw):
    d = _geom(kw)
    return _lib.load().admm_tvd_forward_grouped_record_dev_f32(
        d["y"], d["x"], d["M"], d["N"], d["P"], d["B"], d["gb"], d["gp"], d["h"], d["kh"], d["kw"], d["lam"], d["rho"],
        d["nparam"], d["iso"], d["maxit"], d["flags"], d["ws"], d["ws_bytes"], None)


def _backward(fn, **kw):
    d = _geom(kw)
    return getattr(_lib.load(), fn)(
        d["y"], d["x_bar"], d["y_bar"], d["h_bar"], d["lam_bar"], d["rho_bar"], d["M"], d["N"], d["P"], d["B"], d["gb"],
        d["gp"], d["h"], d["kh"], d["kw"], d["lam"], d["rho"], d["nparam"], d["iso"], d["maxit"], d["x"], d["ws"],
        d["ws_bytes"], None)


def _shared_refusals(call):
    L = _lib.load()
    assert call(gb=3) == _lib.ADMM_E_INVALID
    assert call(gp=2) == _lib.ADMM_E_INVALID
    assert call(nparam=2) == _lib.ADMM_E_INVALID and b"nparam" in L.admm_last_error()
    assert call(nparam=0) == _lib.ADMM_E_INVALID
    assert call(h=None) == _lib.ADMM_E_INVALID and b"NULL" in L.admm_last_error()
    assert call(lam=None) == _lib.ADMM_E_INVALID
    assert call(rho=None) == _lib.ADMM_E_INVALID
    assert call(y=None) == _lib.ADMM_E_INVALID
    assert call(x=FAKE + 4) == _lib.ADMM_E_INVALID
    assert call(maxit=-1) == _lib.ADMM_E_INVALID
    assert call(iso=1, nparam=6) == _lib.ADMM_E_UNSUPPORTED and b"isotropic" in L.admm_last_error()
    assert call(M=8192) == _lib.ADMM_E_UNSUPPORTED
    assert call(B=65281, P=1, gb=1, gp=1, nparam=1) == _lib.ADMM_E_UNSUPPORTED
    assert call(ws_bytes=1024) == _lib.ADMM_E_WORKSPACE
    assert call(ws=FAKE + 8) == _lib.ADMM_E_WORKSPACE
    assert call(ws=None) == _lib.ADMM_E_WORKSPACE


def test_record_refusals_before_any_device_work():
    _shared_refusals(_record)
    assert _record(flags=4) == _lib.ADMM_E_INVALID


@pytest.mark.parametrize("fn", ["admm_tvd_backward_grouped_dev_f32", "admm_tvd_backward_grouped_recorded_dev_f32"])
def test_backward_refusals_before_any_device_work(fn):
    call = lambda **kw: _backward(fn, **kw)   # noqa: E731
    _shared_refusals(call)
    assert call(x_bar=None) == _lib.ADMM_E_INVALID and b"x_bar" in _lib.load().admm_last_error()
    assert call(x_bar=FAKE + 4) == _lib.ADMM_E_INVALID
    assert call(y_bar=FAKE + 4) == _lib.ADMM_E_INVALID and b"y_bar" in _lib.load().admm_last_error()


def test_replay_of_a_workspace_without_a_recording_is_refused():
    L = _lib.load()
    ws = FAKE + (77 << 8)   # an address no test records on
    assert _backward("admm_tvd_backward_grouped_recorded_dev_f32", ws=ws) == _lib.ADMM_E_INVALID
    assert b"no recording" in L.admm_last_error()
    # ... and so is the single-solve replay of it
    rc = L.admm_tvd_backward_recorded_dev_f32(FAKE, FAKE, FAKE, None, FAKE, FAKE, 64, 32, 3, 2, FAKE, 5, 5, FAKE, FAKE, 0, 5,
                                              FAKE, ws, 1 << 40, None, None)
    assert rc == _lib.ADMM_E_INVALID


def test_grouped_adjoint_path_table():
    q = _lib.query_grouped_paths
    R, B_ = _lib.MODE_RECORD, _lib.MODE_BACKWARD
    assert _lib.get_option("MIN_PLANES") == -1
    # runtime-length shapes: the runtime-length forward and sweeps
    assert q(63, 45, False, 10, 6, 6) == ("runtime", "sweep_runtime")
    assert q(63, 45, False, 10, 6, 6, flags=_lib.REC_HBAR) == ("runtime", "sweep_runtime")
    assert q(33, 50, True, 4, 3, 3) == ("runtime", "sweep_runtime_iso")
    assert q(250, 250, False, 15, 512, 512) == ("runtime", "sweep_runtime")   # never resident or smooth-length
    # 256 x 256 anisotropic: the fused trajectory + the 2-pass sweep from the plane-count rule, without h_bar
    assert q(256, 256, False, 15, 96, 96) == ("fused", "sweep_2pass")
    assert q(256, 256, False, 15, 95, 95) == ("2pass", "sweep_2pass")
    assert q(256, 256, False, 15, 96, 96, flags=_lib.REC_HBAR) == ("2pass", "sweep_2pass")
    assert q(256, 256, False, 15, 96, 96, flags=_lib.REC_MASKS) == ("fused", "sweep_2pass")   # not honoured
    assert q(256, 256, False, 15, 96, 2, mode=B_, want_hbar=True) == ("2pass", "sweep_2pass")
    assert q(256, 256, False, 15, 96, 2, mode=B_, want_hbar=False, want_rho=True) == ("fused", "sweep_2pass")
    assert q(256, 256, False, 0, 96, 2, flags=_lib.REC_HBAR) == ("fused", "sweep_2pass")      # no PSF: no h_bar
    assert q(256, 256, True, 15, 512, 4) == ("2pass_iso", "sweep_2pass_iso")
    with _lib.option("FUSED", 0):
        assert q(256, 256, False, 15, 96, 96) == ("2pass", "sweep_2pass")
    with _lib.option("MIN_PLANES", 0):
        assert q(256, 256, False, 15, 4, 2) == ("fused", "sweep_2pass")
        assert q(256, 256, False, 15, 4, 2, flags=_lib.REC_HBAR) == ("2pass", "sweep_2pass")
    # the other tuned shapes
    assert q(64, 32, False, 5, 4, 2) == ("2pass", "sweep_2pass")
    assert q(64, 32, True, 5, 4, 2) == ("2pass_iso", "sweep_2pass_iso")
    # the plain forward: admm_query_grouped_path, no sweep
    assert q(256, 256, False, 15, 96, 96, mode=_lib.MODE_FORWARD) == ("fused", None)
    assert R == 1
    L = _lib.load()
    f, b = ctypes.c_int(0), ctypes.c_int(0)
    assert L.admm_query_grouped_paths(256, 256, 0, 15, 96, 96, 1, 0, 0, 0, None, ctypes.byref(b)) == _lib.ADMM_E_INVALID
    assert L.admm_query_grouped_paths(256, 256, 0, 15, 96, 0, 1, 0, 0, 0, ctypes.byref(f), ctypes.byref(b)) == _lib.ADMM_E_INVALID
    assert L.admm_query_grouped_paths(256, 256, 0, 15, 4, 5, 1, 0, 0, 0, ctypes.byref(f), ctypes.byref(b)) == _lib.ADMM_E_INVALID
    assert L.admm_query_grouped_paths(256, 256, 0, 15, 4, 2, 7, 0, 0, 0, ctypes.byref(f), ctypes.byref(b)) == _lib.ADMM_E_INVALID
    assert L.admm_query_grouped_paths(8192, 256, 0, 15, 4, 2, 1, 0, 0, 0, ctypes.byref(f), ctypes.byref(b)) == _lib.ADMM_E_UNSUPPORTED
