"""Per-plane isotropic mode (isotropic="plane", ADMM_ISO_PLANE), everything that needs no GPU: the oracle of the mode
(tests/plane_bt_oracle.py) and what gives the GPU parity test its teeth, the restated reverse sweep against autograd,
the adjoint cases' distance from the kink of the prox, the C ABI's host side and the Python argument mapping."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_np
import plane_bt_oracle as pbo
import state_oracle
from admm_deconv import _lib
from plane_bt_cases import ADJ_CASES, FWD_CASES, FWD_SEED, K_ADJ, case_id, fwd_K

LAM, RHO = pbo.LAM, pbo.RHO


@functools.lru_cache(maxsize=None)
def _fwd(case):
    B, P, N, M, k = case
    y, _, h = pbo.inputs(B, P, N, M, k, FWD_SEED)
    st = {}
    ref = pbo.solve_loop(y, LAM, RHO, h, fwd_K(case), stats=st)
    return y, h, ref, st["nonzero"]


@pytest.mark.parametrize("case", FWD_CASES, ids=case_id)
def test_loop_and_direct_form_agree(case):
    y, h, ref, _ = _fwd(case)
    d = pbo.solve_direct(y, LAM, RHO, h, fwd_K(case))
    assert pbo.worst_plane_rel(d, ref) <= 1e-13


@pytest.mark.parametrize("case", FWD_CASES, ids=case_id)
def test_single_plane_is_the_reference_isotropic_solve(case):
    """B = P = 1: pixelnorm over 'the whole batch' is the plane's own two channels -- the mode is the reference's."""
    y, h, ref, _ = _fwd(case)
    y1 = y[:1, :1]
    lit = oracle_np.to_c(oracle_np.tvd_fft_literal(oracle_np.from_c(np.asarray(y1, np.float64)), np.float32(LAM),
                                                   np.float32(RHO), oracle_np.psf_from_c(h), True, fwd_K(case)))
    assert np.array_equal(lit[0, 0], ref[0, 0])


@pytest.mark.parametrize("case", FWD_CASES, ids=case_id)
def test_both_prox_branches_are_taken(case):
    _, _, _, nz = _fwd(case)
    print(f"{case_id(case)}: z != 0 in {nz:.1%} of elements")
    assert nz >= 0.01 and 1.0 - nz >= 0.01, f"z != 0 in {nz:.2%}: one branch of the prox is (almost) never taken"


@pytest.mark.parametrize("case", FWD_CASES, ids=case_id)
def test_float32_evaluation_leaves_headroom(case):
    """The oracle's own float32 evaluation against fp64: what fp32 arithmetic costs the algorithm on these inputs, well
    under the 1e-5 parity criterion."""
    y, h, ref, _ = _fwd(case)
    x32 = pbo.solve_loop(y, LAM, RHO, h, fwd_K(case), dtype=np.float32)
    e = pbo.worst_plane_rel(x32, ref)
    print(f"{case_id(case)}: float32 evaluation rel-L2 {e:.2e}")
    assert e <= 1e-6


@pytest.mark.parametrize("case", FWD_CASES, ids=case_id)
def test_other_proxes_are_far_away(case):
    """The batch-coupled isotropic oracle and the anisotropic one on the same inputs: a library that ran either (the
    parent ran the first for isotropic="plane") cannot pass the parity test."""
    y, h, ref, _ = _fwd(case)
    K = fwd_K(case)
    batch = state_oracle.solve(y, LAM, RHO, h, iso=True, K=K)["x"]
    aniso = state_oracle.solve(y, LAM, RHO, h, iso=False, K=K)["x"]
    eb, ea = pbo.rel_l2(batch, ref), pbo.rel_l2(aniso, ref)
    print(f"{case_id(case)}: batch-coupled {eb:.2e}, anisotropic {ea:.2e} away")
    assert eb >= 1e-2 and ea >= 1e-2


@pytest.mark.parametrize("case,seed", [ADJ_CASES[1], ADJ_CASES[3]], ids=lambda v: case_id(v) if isinstance(v, tuple) else str(v))
def test_restated_sweep_equals_autograd(case, seed):
    """kernel_model.tvd_model_grads(iso=True) on one plane at a time, summed, against torch fp64 autograd of the oracle."""
    B, P, N, M, k = case
    y, xbar, h = pbo.inputs(B, P, N, M, k, seed)
    ref = pbo.grads_loop(y, LAM, RHO, h, K_ADJ, xbar)
    got = pbo.model_grads(y, LAM, RHO, h, K_ADJ, xbar)
    assert pbo.rel_l2(got[0], ref[0]) <= 1e-9
    assert pbo.rel_l2(got[1], ref[1]) <= 1e-9
    if h is not None:
        assert pbo.rel_l2(got[2], ref[2]) <= 1e-9
    assert abs(got[3] - ref[3]) <= 1e-9 * abs(ref[3])
    assert abs(got[4] - ref[4]) <= 1e-9 * abs(ref[4])


@pytest.mark.parametrize("case,seed", ADJ_CASES, ids=lambda v: case_id(v) if isinstance(v, tuple) else str(v))
def test_adjoint_cases_stay_off_the_kink(case, seed):
    B, P, N, M, k = case
    y, _, h = pbo.inputs(B, P, N, M, k, seed)
    m = pbo.margin(y, LAM, RHO, h, K_ADJ)
    print(f"{case_id(case)} seed {seed}: min | |s_k| - tau | = {m:.2e}")
    assert m >= 1e-5


# ---- C ABI, host side -------------------------------------------------------------------------------------------
ISO_PLANE = 2


def _ws(L, fn, *args):
    out = ctypes.c_size_t(0)
    return fn(*args, ctypes.byref(out)), out.value


def test_export_and_abi_version():
    L = _lib.load()
    assert "admm_iso_plane_supported" in _lib.EXPORTS
    assert L.admm_iso_plane_supported() == 1
    assert L.admm_abi_version() == 3
    assert (_lib.ISO_NONE, _lib.ISO_BATCH, _lib.ISO_PLANE) == (0, 1, 2)


def test_forward_has_no_plane_limit():
    L = _lib.load()
    rc2, b2 = _ws(L, L.admm_tvd_workspace_bytes, 4, 4, 1, 70000, 0, 0, ISO_PLANE)
    rc0, b0 = _ws(L, L.admm_tvd_workspace_bytes, 4, 4, 1, 70000, 0, 0, 0)
    rc1, _ = _ws(L, L.admm_tvd_workspace_bytes, 4, 4, 1, 70000, 0, 0, 1)
    assert rc2 == _lib.ADMM_OK and rc0 == _lib.ADMM_OK and b2 == b0 > 0
    assert rc1 == _lib.ADMM_E_UNSUPPORTED
    assert b"65535" in L.admm_last_error()
    # the adjoint keeps its per-call limit, as the anisotropic one does
    rc, _ = _ws(L, L.admm_tvd_backward_workspace_bytes, 4, 4, 1, 70000, 0, 0, ISO_PLANE, 3, 0)
    assert rc == _lib.ADMM_E_UNSUPPORTED


@pytest.mark.parametrize("shape", [(256, 256, 15), (64, 32, 5), (250, 250, 15), (480, 640, 0), (30, 40, 5)])
def test_workspace_is_the_anisotropic_layout(shape):
    L = _lib.load()
    M, N, k = shape
    for fn, tail in ((L.admm_tvd_workspace_bytes, ()), (L.admm_tvd_backward_workspace_bytes, (4, 1)),
                     (L.admm_tvd_backward_workspace_bytes, (4, 0))):
        rc2, b2 = _ws(L, fn, M, N, 3, 2, k, k, ISO_PLANE, *tail)
        assert rc2 == _lib.ADMM_OK, L.admm_last_error()
        # the anisotropic layout of the same path: the 2-pass / runtime-length one (no fmap, part or nrm slots)
        with _lib.option("FUSED", 0), _lib.option("SMOOTH", 0), _lib.option("RESIDENT", 0), _lib.option("MALL_STREAMS", 1):
            rc0, b0 = _ws(L, fn, M, N, 3, 2, k, k, 0, *tail)
        assert rc0 == _lib.ADMM_OK and b2 == b0, (b2, b0)
    rc2, g2 = _ws(L, L.admm_tvd_grouped_workspace_bytes, M, N, 3, 2, 2, 3, k, k, ISO_PLANE)
    rc0, g0 = _ws(L, L.admm_tvd_grouped_workspace_bytes, M, N, 3, 2, 2, 3, k, k, 0)
    assert rc2 == rc0 == _lib.ADMM_OK and g2 == g0


def _paths(L, M, N, iso, planes, mode, kh=15):
    f, b = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = L.admm_query_paths(M, N, iso, kh, planes, mode, 0, 0, 1, ctypes.byref(f), ctypes.byref(b))
    assert rc == _lib.ADMM_OK, L.admm_last_error()
    return L.admm_path_name(f.value).decode(), L.admm_path_name(b.value).decode()


def test_paths_of_the_mode():
    L = _lib.load()
    L.admm_path_name.restype = ctypes.c_char_p
    before = {(M, N, pl, iso, mode): _paths(L, M, N, iso, pl, mode)
              for (M, N, pl) in ((256, 256, 512), (250, 250, 256), (640, 480, 64)) for iso in (0, 1)
              for mode in (_lib.MODE_FORWARD, _lib.MODE_RECORD, _lib.MODE_BACKWARD)}
    for mode in (_lib.MODE_RECORD, _lib.MODE_BACKWARD):
        assert _paths(L, 256, 256, ISO_PLANE, 512, mode) == ("2pass", "sweep_2pass")
        assert _paths(L, 250, 250, ISO_PLANE, 256, mode) == ("runtime", "sweep_runtime")
        assert _paths(L, 640, 480, ISO_PLANE, 64, mode) == ("runtime", "sweep_runtime")
    assert _paths(L, 256, 256, ISO_PLANE, 512, _lib.MODE_FORWARD) == ("2pass", "none")
    assert _paths(L, 250, 250, ISO_PLANE, 256, _lib.MODE_FORWARD) == ("runtime", "none")
    assert _paths(L, 640, 480, ISO_PLANE, 64, _lib.MODE_FORWARD)[0] == "runtime"
    # whatever the plane count: a plane's path (and so its bits) never depends on its batch
    assert _paths(L, 256, 256, ISO_PLANE, 1, _lib.MODE_FORWARD) == _paths(L, 256, 256, ISO_PLANE, 0, _lib.MODE_FORWARD)
    # iso = 0 and 1 answer as before the mode was asked about, and as the documented table says
    assert before[(256, 256, 512, 0, _lib.MODE_FORWARD)] == ("fused", "none")
    assert before[(256, 256, 512, 1, _lib.MODE_FORWARD)] == ("fused_iso", "none")
    assert before[(250, 250, 256, 0, _lib.MODE_FORWARD)][0] == "resident"
    for key, val in before.items():
        assert _paths(L, key[0], key[1], key[3], key[2], key[4]) == val
    # any non-zero value but 2 keeps meaning the batch-coupled prox
    assert _paths(L, 256, 256, 3, 512, _lib.MODE_FORWARD) == before[(256, 256, 512, 1, _lib.MODE_FORWARD)]
    assert _paths(L, 256, 256, -1, 512, _lib.MODE_FORWARD) == before[(256, 256, 512, 1, _lib.MODE_FORWARD)]


def test_schedule_and_grouped_path():
    L = _lib.load()
    c, n = ctypes.c_longlong(0), ctypes.c_int(0)
    # c4's batch: the anisotropic solve takes the MALL chunk schedule, the mode plain chunks
    assert L.admm_query_forward_schedule(512, 512, ISO_PLANE, 0, 768, ctypes.byref(c), ctypes.byref(n)) == _lib.ADMM_OK
    assert (c.value, n.value) == (768, 1)
    assert L.admm_query_forward_schedule(4, 2, ISO_PLANE, 0, 65300, ctypes.byref(c), ctypes.byref(n)) == _lib.ADMM_OK
    assert (c.value, n.value) == (65280, 1)
    f = ctypes.c_int(-1)
    assert L.admm_query_grouped_path(256, 256, ISO_PLANE, 5, 512, 4, ctypes.byref(f)) == _lib.ADMM_OK
    L.admm_path_name.restype = ctypes.c_char_p
    assert L.admm_path_name(f.value) == b"2pass"
    assert L.admm_query_grouped_path(40, 30, ISO_PLANE, 5, 4, 4, ctypes.byref(f)) == _lib.ADMM_OK
    assert L.admm_path_name(f.value) == b"runtime"


def test_entry_points_without_the_mode_refuse_it():
    L = _lib.load()
    out = ctypes.c_size_t(0)
    f, b = ctypes.c_int(0), ctypes.c_int(0)
    fake = ctypes.c_void_p(4096)   # never dereferenced: the mode is refused before anything is read
    calls = {
        "state workspace": lambda iso: L.admm_tvd_state_workspace_bytes(32, 32, 1, 2, 0, 0, iso, ctypes.byref(out)),
        "state path": lambda iso: L.admm_query_state_path(32, 32, iso, 0, 2, ctypes.byref(f)),
        "grouped adjoint workspace": lambda iso: L.admm_tvd_grouped_backward_workspace_bytes(
            32, 32, 1, 2, 2, 1, 0, 0, iso, 3, 0, ctypes.byref(out)),
        "grouped adjoint paths": lambda iso: L.admm_query_grouped_paths(32, 32, iso, 0, 2, 2, _lib.MODE_RECORD, 0, 0, 0,
                                                                        ctypes.byref(f), ctypes.byref(b)),
    }
    for name, call in calls.items():
        assert call(ISO_PLANE) == _lib.ADMM_E_UNSUPPORTED, name
        assert b"ADMM_ISO_PLANE" in L.admm_last_error(), name
        assert call(0) == _lib.ADMM_OK and call(1) == _lib.ADMM_OK, name
    rc = L.admm_tvd_forward_state_dev_f32(fake, fake, 32, 32, 1, 2, None, 0, 0, fake, fake, ISO_PLANE, 3, None, None, None,
                                          fake, 1 << 20, None)
    assert rc == _lib.ADMM_E_UNSUPPORTED and b"ADMM_ISO_PLANE" in L.admm_last_error()
    rc = L.admm_tvd_forward_grouped_record_dev_f32(fake, fake, 32, 32, 1, 2, 2, 1, None, 0, 0, fake, fake, 1, ISO_PLANE, 3,
                                                   0, fake, 1 << 20, None)
    assert rc == _lib.ADMM_E_UNSUPPORTED and b"ADMM_ISO_PLANE" in L.admm_last_error()


# ---- Python argument mapping --------------------------------------------------------------------------------------
def test_isotropic_argument_maps_to_one_code():
    assert _lib.iso_code(False) == 0 and _lib.iso_code(True) == 1 and _lib.iso_code("plane") == 2
    assert _lib.iso_code(0) == 0 and _lib.iso_code(1) == 1 and _lib.iso_code(None) == 0   # as int(bool(.)) before
    assert _lib.iso_code(np.bool_(True)) == 1
    for bad in ("Plane", "batch", "", "true"):
        with pytest.raises(ValueError):
            _lib.iso_code(bad)
    assert _lib.workspace_bytes(64, 64, 1, 2, 0, 0, "plane") == _lib.workspace_bytes(64, 64, 1, 2, 0, 0, False)
    assert _lib.workspace_bytes(64, 64, 1, 2, 0, 0, True) > _lib.workspace_bytes(64, 64, 1, 2, 0, 0, False)
    assert _lib.query_paths(256, 256, "plane", planes=512) == _lib.query_paths(256, 256, False, planes=1)


def test_entry_points_without_the_mode_raise():
    from admm_deconv import ops
    for fn, args in ((ops.tvd_fft_state, (None, 0.05, 0.1, None, "plane", 3)),
                     (ops.tvd_fft_tol, (None, 0.05, 0.1, None, "plane", 3)),
                     (ops.tvd_fft_grouped_record, (None, 0.05, 0.1, None, "plane", 3)),
                     (ops.tvd_fft_grouped_backward, (None, None, 0.05, 0.1, None, "plane", 3)),
                     (ops.tvd_fft_grouped_grad, (None, 0.05, 0.1, None, "plane", 3))):
        with pytest.raises(ValueError, match="plane"):
            fn(*args)
    with pytest.raises(ValueError, match="plane"):
        ops.tvd_fft_multi(None, [0.05], [0.1], 3, isotropic="plane")
    with pytest.raises(ValueError, match="plane"):
        ops.tvd_fft_multi_grad(None, [0.05], [0.1], 3, isotropic="plane")
    assert ops.multi_supported(None, "plane") is False
    assert ops._sharded("plane", object()) is False   # group= is ignored: nothing crosses planes


def test_layers_take_the_mode():
    from admm_deconv import layers
    for cls, args in ((layers.ADMMDeconv, ((5, 5), 4)), (layers.ADMMDeconvF1, ((5, 5), 4, 0.05)),
                      (layers.ADMMDeconvF2, ((5, 5), 4, 0.1)), (layers.ADMMDeconvF3, ((5, 5), 4, 0.05, 0.1))):
        d = cls(*args, iso="plane", device="cpu")
        assert d.iso == "plane" and "iso='plane'" in repr(d)
        assert cls(*args, iso=True, device="cpu").iso is True and "iso=True" in repr(cls(*args, iso=True, device="cpu"))
        with pytest.raises(ValueError):
            cls(*args, iso="batch", device="cpu")
    a, b = (layers.ADMMDeconvF2((), 4, 0.1, iso="plane", device="cpu") for _ in range(2))
    assert layers.Parallel(layers.chcat, a, b)._mergeable(None) is False
