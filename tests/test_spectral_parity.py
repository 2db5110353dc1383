"""CPU: the length sweep's lists, teeth and margins (tests/spectral_parity.py, tests/test_gpu_length_sweep.py).

List sync: the helper's length lists are admm_smooth.hip's, so a length compiled later cannot go unswept.  Teeth: a 1e-3
relative error in one bin pair of the oracle's own x exceeds every case's per-bin bound with the committed constants --
and, at the long shapes, passes the plane-wide parity criterion, which is the hole the sweep closes.  Margins: every
case's prox is live, and every adjoint case's masks are at least 1e-5 from flipping, from the oracle alone."""
import os
import re

import numpy as np
import pytest

import parity
import spectral_parity as sp

SMOOTH_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "admm-deconv_amd", "csrc",
                          "admm_smooth.hip")
FORWARD = sp.forward_cases()
ADJOINT = sp.adjoint_cases()


def _macro_lengths(name):
    src = open(SMOOTH_SRC).read()
    m = re.search(r"#define\s+" + name + r"\(X\)((?:[^\n]*\\\n)*[^\n]*)", src)
    assert m, f"{name} not found in admm_smooth.hip"
    return tuple(int(v) for v in re.findall(r"X\((\d+)\)", m.group(1)))


def test_length_lists_are_the_sources():
    assert _macro_lengths("SM_LENGTHS") == sp.COMPILED_LENGTHS
    assert _macro_lengths("SM_COL_ASC_LENGTHS") == sp.COL_ASC_LENGTHS
    assert set(sp.COL_ASC_LENGTHS) <= set(sp.COMPILED_LENGTHS)


def test_every_compiled_length_is_swept_in_both_roles_and_orders():
    seen = {(c.role, c.L, c.smooth) for c in sp.compiled_cases()}
    for L in sp.COMPILED_LENGTHS:
        other = 3 if L in sp.COL_ASC_LENGTHS else 2
        assert {("line", L, None), ("column", L, None), ("column", L, other)} <= seen
    ids = [c.id for c in FORWARD + ADJOINT]
    assert len(ids) == len(set(ids))
    assert all(c.path == "smooth" and c.R == 0 for c in sp.compiled_cases())
    assert all(c.path == "runtime" for c in sp.runtime_cases())


def test_runtime_families():
    assert sp.factors(4095) == [3, 3, 5, 7, 13] and sp.factors(3072) == [8, 8, 8, 2, 3] and sp.factors(2039) == [2039]
    assert sp.factors(96) == [8, 4, 3] and sp.factors(4094) == [2, 23, 89]
    assert sp.direct_factor(3993) == 11 and sp.direct_factor(4000) == 0 and sp.direct_factor(221) == 17


def _mutations(N, M):
    """a low bin, and each side's last bin"""
    return [(N // 3, M // 3), (N // 3, M // 2), (N // 2, M // 3)]


@pytest.mark.parametrize("case", FORWARD, ids=lambda c: c.id)
def test_teeth_and_margins(case):
    frac = parity.assert_prox_active(sp.prox_fraction(case), case.id)
    x = sp.oracle(case)[0]["x"]
    b = sp.bound(case)
    for j, k in _mutations(case.N, case.M):
        xm = sp.mutate_bin(x, j, k)
        e = sp.bin_error(xm, x)
        assert e > b, (f"{case.id}: a 1e-3 error in bin ({j}, {k}) moves the per-bin figure by {e:.2e}, inside the bound "
                       f"{b:.2e} (prox fraction {frac:.2f})")
        if max(case.N, case.M) >= 1000:
            parity.assert_parity(xm, x, what=f"{case.id}: the mutated oracle under the plane-wide criterion")


@pytest.mark.parametrize("case", ADJOINT, ids=lambda c: c.id)
def test_adjoint_margins(case):
    parity.assert_prox_active(sp.prox_fraction(case), case.id)
    m = sp.threshold_margin(case)
    assert m >= 1e-5, f"{case.id}: an oracle |s_k| is {m:.2e} from tau: fp32 may flip that mask (another seed)"


def test_bin_error_is_per_plane_and_scale_free():
    rng = np.random.default_rng(5)
    ref = rng.standard_normal((2, 1, 9, 18))
    got = ref.copy()
    got[1, 0] = sp.mutate_bin(ref[1, 0], 3, 6, rel=1e-2)
    e = sp.bin_error(got, ref)
    R = np.abs(np.fft.fft2(ref[1, 0]))
    assert np.isclose(e, 1e-2 * R[3, 6] / np.sqrt(np.mean(R * R)), rtol=1e-9)
    assert np.isclose(sp.bin_error(10 * got, 10 * ref), e, rtol=1e-12) and sp.bin_error(ref, ref) == 0.0
