"""CPU: host-side AddressSanitizer run of the resumable solve's C ABI.

__graft_entry__.build() builds tests/asan/state_host_check.c against the instrumented library of tests/test_asan.py
(admm-deconv_amd/asan/): a stand-alone, GPU-free driver of the state call's validation, workspace sweep and path query.
Nothing is preloaded into Python; ASan aborts the driver on any out-of-bounds access, use-after-free or leak."""
import os
import subprocess

ASAN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "admm-deconv_amd", "asan")


def test_state_host_paths_under_asan():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:detect_stack_use_after_return=1")
    r = subprocess.run([os.path.join(ASAN, "state_host_check")], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "asan state host check: ok" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "ERROR: LeakSanitizer" not in r.stderr
