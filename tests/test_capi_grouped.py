"""CPU: the grouped solve's C ABI (include/admm_deconv.h) -- exports, workspace size, argument refusals and the path
decision.  No GPU work is issued: every refusal comes before the first launch."""
import ctypes
import os
import re

import pytest

from admm_deconv import _lib

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "admm_deconv.h")
NAMES = ("admm_tvd_grouped_workspace_bytes", "admm_tvd_forward_grouped_dev_f32", "admm_query_grouped_path")
FAKE = 1 << 20   # a "device pointer" that is never dereferenced: validation fails first


def test_header_binding_and_library_export_the_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    L = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert n in _lib.EXPORTS, n
        assert hasattr(L, n), n
    assert L.admm_abi_version() == 3   # symbols were added only


def test_workspace_grows_with_the_group_count():
    one = _lib.grouped_workspace_bytes(256, 256, 2, 8, 1, 1, 15, 15, False)
    per_image = _lib.grouped_workspace_bytes(256, 256, 2, 8, 8, 1, 15, 15, False)
    per_plane = _lib.grouped_workspace_bytes(256, 256, 2, 8, 8, 2, 15, 15, False)
    assert _lib.workspace_bytes(256, 256, 2, 8, 15, 15, False) < one < per_image < per_plane
    # a group costs its C and G tables (129 x 256 bins, 4 + 8 B), its lane-native tables and a scalar block
    per_group = (per_plane - per_image) / 8
    assert 129 * 256 * 12 + 32768 * 12 <= per_group <= 129 * 256 * 12 + 32768 * 12 + 8192
    # no PSF: no G tables; runtime-length shapes: no lane-native tables
    assert _lib.grouped_workspace_bytes(256, 256, 2, 8, 8, 2, 0, 0, False) < per_plane
    g1, g6 = (_lib.grouped_workspace_bytes(63, 45, 3, 2, gb, gp, 5, 5, True) for gb, gp in ((1, 1), (2, 3)))
    assert 5 * 32 * 45 * 12 <= g6 - g1 <= 5 * 32 * 45 * 12 + 5 * 1024


@pytest.mark.parametrize("args,code", [
    ((64, 32, 3, 2, 3, 1, 5, 5, 0), _lib.ADMM_E_INVALID),        # gb neither 1 nor B
    ((64, 32, 3, 2, 1, 2, 5, 5, 0), _lib.ADMM_E_INVALID),        # gp neither 1 nor P
    ((64, 32, 3, 2, 0, 1, 5, 5, 0), _lib.ADMM_E_INVALID),
    ((64, 32, 3, 2, 2, 3, 5, 0, 0), _lib.ADMM_E_INVALID),        # half-empty PSF
    ((8192, 32, 3, 2, 2, 3, 5, 5, 0), _lib.ADMM_E_UNSUPPORTED),  # shapes as check_shape
    ((64, 32, 3, 2, 2, 3, 65, 5, 0), _lib.ADMM_E_UNSUPPORTED),   # kh > M
    ((8, 8, 1, 65281, 1, 1, 3, 3, 0), _lib.ADMM_E_UNSUPPORTED),  # above 65,280 planes: no internal chunking
])
def test_workspace_query_refusals(args, code):
    out = ctypes.c_size_t(0)
    L = _lib.load()
    assert L.admm_tvd_grouped_workspace_bytes(*args, ctypes.byref(out)) == code
    assert len(L.admm_last_error()) > 0
    assert L.admm_tvd_grouped_workspace_bytes(64, 32, 3, 2, 2, 3, 5, 5, 0, None) == _lib.ADMM_E_INVALID


def test_most_planes_of_one_call():
    assert _lib.grouped_workspace_bytes(8, 8, 1, 65280, 65280, 1, 3, 3, False) > 0


def _call(M=64, N=32, P=3, B=2, gb=2, gp=3, h=FAKE, kh=5, kw=5, lam=FAKE, rho=FAKE, nparam=6, iso=0, maxit=5, y=FAKE,
          x=FAKE, ws=FAKE, ws_bytes=1 << 40):
    return _lib.load().admm_tvd_forward_grouped_dev_f32(y, x, M, N, P, B, gb, gp, h, kh, kw, lam, rho, nparam, iso, maxit,
                                                        ws, ws_bytes, None)


def test_forward_refusals_before_any_device_work():
    L = _lib.load()
    assert _call(gb=3) == _lib.ADMM_E_INVALID
    assert _call(gp=2) == _lib.ADMM_E_INVALID
    assert _call(nparam=2) == _lib.ADMM_E_INVALID and b"nparam" in L.admm_last_error()
    assert _call(nparam=0) == _lib.ADMM_E_INVALID
    assert _call(h=None) == _lib.ADMM_E_INVALID and b"NULL" in L.admm_last_error()
    assert _call(lam=None) == _lib.ADMM_E_INVALID
    assert _call(rho=None) == _lib.ADMM_E_INVALID
    assert _call(y=None) == _lib.ADMM_E_INVALID
    assert _call(maxit=-1) == _lib.ADMM_E_INVALID
    # the isotropic prox is one BT factor map per batch: one (lambda, rho) pair
    assert _call(iso=1, nparam=6) == _lib.ADMM_E_UNSUPPORTED and b"isotropic" in L.admm_last_error()
    assert _call(M=8192) == _lib.ADMM_E_UNSUPPORTED
    assert _call(B=65281, P=1, gb=1, gp=1, nparam=1) == _lib.ADMM_E_UNSUPPORTED
    assert _call(ws_bytes=1024) == _lib.ADMM_E_WORKSPACE
    assert _call(ws=FAKE + 8) == _lib.ADMM_E_WORKSPACE
    assert _call(ws=None) == _lib.ADMM_E_WORKSPACE


def test_grouped_path_decision():
    q = _lib.query_grouped_path
    assert _lib.get_option("MIN_PLANES") == -1
    assert q(256, 256, False, 15, 96, 96) == "fused"
    assert q(256, 256, False, 15, 95, 95) == "2pass"          # below the fused kernel's plane count
    assert q(256, 256, False, 0, 512, 2) == "fused"
    assert q(256, 256, True, 15, 512, 1) == "2pass_iso"       # the fused isotropic kernels take one table set
    assert q(64, 32, False, 5, 4, 2) == "2pass"
    assert q(64, 32, True, 5, 4, 2) == "2pass_iso"
    assert q(63, 45, False, 5, 6, 6) == "runtime"
    assert q(63, 45, True, 5, 6, 6) == "runtime"
    assert q(250, 250, False, 15, 512, 512) == "runtime"      # never the resident or smooth-length kernels
    assert q(640, 480, False, 15, 64, 64) == "runtime"
    with _lib.option("MIN_PLANES", 0):
        assert q(256, 256, False, 15, 6, 3) == "fused"
    with _lib.option("FUSED", 0):
        assert q(256, 256, False, 15, 96, 96) == "2pass"
    L = _lib.load()
    f = ctypes.c_int(0)
    assert L.admm_query_grouped_path(256, 256, 0, 15, 96, 96, None) == _lib.ADMM_E_INVALID
    assert L.admm_query_grouped_path(256, 256, 0, 15, 96, 0, ctypes.byref(f)) == _lib.ADMM_E_INVALID
    assert L.admm_query_grouped_path(256, 256, 0, 15, 4, 5, ctypes.byref(f)) == _lib.ADMM_E_INVALID
    assert L.admm_query_grouped_path(8192, 256, 0, 15, 4, 2, ctypes.byref(f)) == _lib.ADMM_E_UNSUPPORTED


def test_python_entry_rejects_host_tensors():
    import torch
    from admm_deconv import tvd_fft_grouped
    with pytest.raises(TypeError):
        tvd_fft_grouped(torch.zeros(2, 3, 8, 8), 0.1, 1.0, None)
