"""CPU: the resumable solve's C ABI (include/admm_deconv.h) -- exports, workspace size, argument refusals and the path
decision.  No GPU work is issued: every refusal comes before the first launch."""
import ctypes
import os
import re

import pytest

from admm_deconv import _lib

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "admm_deconv.h")
NAMES = ("admm_tvd_state_workspace_bytes", "admm_tvd_forward_state_dev_f32", "admm_query_state_path")
FAKE = 1 << 20   # a "device pointer" that is never dereferenced: validation fails first


def test_header_binding_and_library_export_the_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    L = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert n in _lib.EXPORTS, n
        assert hasattr(L, n), n
    assert L.admm_abi_version() == 3   # symbols were added only


@pytest.mark.parametrize("shape", [(256, 256), (64, 64), (32, 128), (16, 8), (96, 96), (250, 250), (40, 30), (33, 27),
                                   (512, 512)])
@pytest.mark.parametrize("iso", [0, 1])
@pytest.mark.parametrize("k", [0, 9])
def test_workspace_covers_the_plain_forward_and_is_aligned(shape, iso, k):
    M, N = shape
    k = min(k, M, N)
    for P, B in ((1, 1), (3, 5), (1, 600)):
        w = _lib.state_workspace_bytes(M, N, P, B, k, k, iso)
        assert w % 256 == 0
        assert w >= _lib.workspace_bytes(M, N, P, B, k, k, iso)
        # one v_0 plane set at least on top of the whole batch's forward layout
        assert w >= 4 * M * N * P * B


def test_workspace_query_refusals():
    out = ctypes.c_size_t(0)
    L = _lib.load()
    q = L.admm_tvd_state_workspace_bytes
    assert q(64, 64, 1, 2, 5, 5, 0, None) == _lib.ADMM_E_INVALID
    assert q(8, 8, 1, 65281, 3, 3, 0, ctypes.byref(out)) == _lib.ADMM_E_UNSUPPORTED   # no internal chunking
    assert q(8, 8, 1, 65280, 3, 3, 0, ctypes.byref(out)) == _lib.ADMM_OK and out.value > 0
    assert q(1, 8, 1, 1, 0, 0, 0, ctypes.byref(out)) == _lib.ADMM_E_UNSUPPORTED
    assert q(4097, 8, 1, 1, 0, 0, 0, ctypes.byref(out)) == _lib.ADMM_E_UNSUPPORTED
    assert q(64, 64, 1, 1, 5, 0, 0, ctypes.byref(out)) == _lib.ADMM_E_INVALID           # half-empty PSF


def _call(M=64, N=32, P=3, B=2, h=FAKE, kh=5, kw=5, lam=FAKE, rho=FAKE, iso=0, maxit=5, y=FAKE, x=FAKE, s_in=None,
          s_out=None, resid=None, ws=FAKE, ws_bytes=1 << 40):
    return _lib.load().admm_tvd_forward_state_dev_f32(y, x, M, N, P, B, h, kh, kw, lam, rho, iso, maxit, s_in, s_out,
                                                      resid, ws, ws_bytes, None)


def test_forward_refusals_before_any_device_work():
    L = _lib.load()
    assert _call(maxit=0) == _lib.ADMM_E_INVALID and b"maxit" in L.admm_last_error()
    assert _call(maxit=-1) == _lib.ADMM_E_INVALID
    assert _call(s_in=FAKE, s_out=FAKE) == _lib.ADMM_E_INVALID and b"state_out" in L.admm_last_error()
    assert _call(lam=None) == _lib.ADMM_E_INVALID
    assert _call(rho=None) == _lib.ADMM_E_INVALID
    assert _call(h=None) == _lib.ADMM_E_INVALID and b"NULL" in L.admm_last_error()
    assert _call(y=None) == _lib.ADMM_E_INVALID
    assert _call(x=None) == _lib.ADMM_E_INVALID
    assert _call(B=65281, P=1) == _lib.ADMM_E_UNSUPPORTED and b"65280" in L.admm_last_error()
    assert _call(M=1) == _lib.ADMM_E_UNSUPPORTED
    assert _call(N=1) == _lib.ADMM_E_UNSUPPORTED
    assert _call(M=4097) == _lib.ADMM_E_UNSUPPORTED
    assert _call(N=8192) == _lib.ADMM_E_UNSUPPORTED
    assert _call(s_in=FAKE + 4) == _lib.ADMM_E_INVALID
    # a workspace of the plain forward's size is too small, a misaligned one refused
    assert _call(ws_bytes=_lib.workspace_bytes(64, 32, 3, 2, 5, 5, 0)) == _lib.ADMM_E_WORKSPACE
    assert _call(ws=FAKE + 16) == _lib.ADMM_E_WORKSPACE
    assert _call(ws=None) == _lib.ADMM_E_WORKSPACE


def test_path_table():
    q = _lib.query_state_path
    # 256 x 256 anisotropic: the fused kernel's state instance, from its plane count on
    assert q(256, 256, False, 15, 512) == "fused"
    assert q(256, 256, False, 0, 96) == "fused"
    assert q(256, 256, False, 15, 95) == "2pass"
    assert q(256, 256, False, 15, 0) == "fused"        # planes not known: no plane-count rule
    assert q(256, 256, True, 15, 512) == "2pass_iso"
    assert q(64, 64, False, 9, 512) == "2pass"
    assert q(64, 64, True, 9, 512) == "2pass_iso"
    assert q(32, 128, False, 5, 4) == "2pass"
    # runtime-length shapes, the smooth ones included: never the smooth-length or CU-resident kernels
    for M, N in ((96, 96), (250, 250), (40, 30)):
        for iso in (False, True):
            assert q(M, N, iso, 5, 512) == "runtime"
    with _lib.option("FUSED", 0):
        assert q(256, 256, False, 15, 512) == "2pass"
    with _lib.option("MIN_PLANES", 0):
        assert q(256, 256, False, 15, 2) == "fused"


def test_path_query_refusals():
    L = _lib.load()
    f = ctypes.c_int(0)
    assert L.admm_query_state_path(256, 256, 0, 15, 512, None) == _lib.ADMM_E_INVALID
    assert L.admm_query_state_path(256, 256, 0, 15, -1, ctypes.byref(f)) == _lib.ADMM_E_INVALID
    assert L.admm_query_state_path(256, 256, 0, 15, 65281, ctypes.byref(f)) == _lib.ADMM_E_INVALID
    assert L.admm_query_state_path(1, 256, 0, 0, 4, ctypes.byref(f)) == _lib.ADMM_E_UNSUPPORTED
