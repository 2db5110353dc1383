"""CPU: every workspace size query of the C ABI (admm_tvd_workspace_bytes, _backward_, _grouped_, _grouped_backward_
and _multi_workspace_bytes) returns exactly the byte count committed in tests/golden/workspace_bytes.json, over the
sweep of tests/golden/gen_workspace_bytes.py.  The table was generated from the library before the workspace carver
and the grouped table blocks were written once (admm_capi.hip), so a layout whose total moves by one byte fails here."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gen_workspace_bytes as gen  # noqa: E402


@pytest.fixture(scope="module")
def tables():
    with open(gen.OUT) as f:
        return json.load(f), gen.measure()


def test_the_table_covers_the_sweep(tables):
    want, got = tables
    assert set(want) == set(gen.QUERIES) == set(got)
    n = {name: 0 for name in gen.QUERIES}
    for name, _ in gen.calls():
        n[name] += 1
    assert {k: len(v) for k, v in want.items()} == n
    assert all(v > 0 for name in want for v in want[name]), "a refused query in the pinned sweep"


@pytest.mark.parametrize("name", sorted(gen.QUERIES))
def test_workspace_bytes_are_pinned(tables, name):
    want, got = tables
    args = [a for q, a in gen.calls() if q == name]
    bad = [(a, w, g) for a, w, g in zip(args, want[name], got[name]) if w != g]
    assert not bad, f"{name}: {len(bad)} of {len(args)} byte counts moved; first (arguments, pinned, now): {bad[:3]}"
