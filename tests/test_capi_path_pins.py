"""CPU: every path query of the C ABI (admm_query_paths, _grouped_paths, _grouped_path, _state_path and
_forward_schedule) answers exactly what tests/golden/path_decisions.json holds, over the sweep of
tests/golden/gen_path_decisions.py; so do the multi-branch workspace sizes on both sides of the plane-count rule and
the (code, message) of the calls the multi-branch, grouped and state entry points refuse before any device work.  The
table was generated from the library while plan_paths covered single solves only and plan_grouped,
plan_grouped_adjoint, plan_state and multi_two_pass decided the other families: the one path table must decide as
they did, query by query, and a wrong call must be told the same thing, character for character."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gen_path_decisions as gen  # noqa: E402

from admm_deconv import _lib  # noqa: E402


@pytest.fixture(scope="module")
def table():
    with open(gen.OUT) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def pinned(table):
    return gen.decode(table)


def _name(path):
    return _lib.load().admm_path_name(path).decode()


def _readable(a):
    """An answer with its path codes as names."""
    return a if isinstance(a, int) else [_name(p) if p else None for p in a]


def test_path_decisions_are_pinned(pinned):
    blocks = list(gen.blocks())
    assert len(blocks) == len(pinned)
    n = 0
    for (fam, opts, shape, prox), want in zip(blocks, pinned):
        with gen.options(opts):
            got = json.loads(json.dumps(gen.answers(fam, shape, prox)))
        assert len(got) == len(want), f"{fam} {opts} {shape} prox={prox!r}: {len(want)} pinned queries, {len(got)} now"
        n += len(got)
        if got == want:
            continue
        i = next(i for i, (w, g) in enumerate(zip(want, got)) if w != g)
        q = dict(zip(("kh", "planes", "mode", "rec_flags", "want_hbar", "want_rho"), list(gen.queries(fam, shape))[i]))
        sched = fam.startswith("forward_schedule")
        w, g = (want[i], got[i]) if sched else (_readable(want[i]), _readable(got[i]))
        pytest.fail(f"{fam}, options {opts}, shape {shape}, prox {prox!r}: {sum(a != b for a, b in zip(want, got))} of "
                    f"{len(want)} answers moved; first at query {q}: pinned {w}, now {g}")
    assert n > 700000


def _has(table, pinned, fam, answer, prox=None):
    """Some block of `fam` (of that prox, if given) holds the answer (path names; an int: minus an error code)."""
    show = (lambda a: a) if fam.startswith("forward_schedule") else _readable
    for (f, _, _, p), seq in zip(gen.blocks(), pinned):
        if f == fam and (prox is None or p == prox) and any(show(a) == answer for a in seq):
            return True
    return False


SINGLE = [["fused", "sweep_fused"], ["fused", "sweep_2pass"], ["fused_iso", "sweep_fused_iso"],
          ["resident", "sweep_2pass"], ["resident", "sweep_runtime"], ["resident_iso", "sweep_2pass_iso"],
          ["resident_iso", "sweep_runtime_iso"], ["smooth", "sweep_runtime"], ["smooth", "sweep_runtime_iso"],
          ["runtime", "sweep_runtime"], ["runtime", "sweep_runtime_iso"], ["2pass", "sweep_2pass"],
          ["2pass_iso", "sweep_2pass_iso"]]
GROUPED = [["fused", "sweep_2pass"], ["2pass", "sweep_2pass"], ["2pass_iso", "sweep_2pass_iso"],
           ["runtime", "sweep_runtime"], ["runtime", "sweep_runtime_iso"]]
STATE = [["fused"], ["2pass"], ["2pass_iso"], ["runtime"]]


def test_the_pinned_table_is_not_uniform(table, pinned):
    """The answers the sweep must contain: every forward path of admm_path_name with its sweeps for single solves, the
    grouped and state families' own sets -- and none of the kernels those families cannot take."""
    for a in SINGLE:
        assert _has(table, pinned, "paths", a), f"single: {a} is not in the pinned sweep"
    for a in SINGLE:
        assert _has(table, pinned, "paths", [a[0], None]), f"single: forward {a[0]} is not in the pinned sweep"
    for a in GROUPED:
        assert _has(table, pinned, "grouped_paths", a), f"grouped: {a} is not in the pinned sweep"
    assert _has(table, pinned, "grouped_paths", _lib.ADMM_E_UNSUPPORTED, "plane"), "grouped adjoint: no \"plane\" refusal"
    assert _has(table, pinned, "grouped_paths", ["2pass", None], "plane") and _has(table, pinned, "grouped_path", ["2pass"],
                                                                                  "plane")
    for a in STATE:
        assert _has(table, pinned, "state_path", a), f"state: {a} is not in the pinned sweep"
    assert _has(table, pinned, "state_path", _lib.ADMM_E_UNSUPPORTED, "plane"), "state: no \"plane\" refusal"
    never = {"smooth", "resident", "resident_iso", "fused_iso", "sweep_fused", "sweep_fused_iso"}
    for (fam, opts, shape, prox), seq in zip(gen.blocks(), pinned):
        if fam in ("grouped_paths", "grouped_path", "state_path"):
            seen = {n for a in seq if not isinstance(a, int) for n in _readable(a)}
            assert not (seen & never), f"{fam} {opts} {shape} {prox!r}: pinned {seen & never}"
    # the MALL schedule, and its absence
    assert _has(table, pinned, "forward_schedule_mall4", [8, 4]) and _has(table, pinned, "forward_schedule_mall4", [768, 1])


def test_multi_workspace_bytes_are_pinned(table):
    """Both grids of the multi-branch family (fused from the plane-count rule on, 2-pass below) have their own layout:
    the byte counts show which one was planned."""
    want, got = table["multi_bytes"], gen.multi_bytes()
    calls = list(gen.multi_calls())
    assert len(want) == len(calls) == len(got)
    bad = [(c, w, g) for c, w, g in zip(calls, want, got) if w != g]
    assert not bad, f"{len(bad)} of {len(calls)} byte counts moved; first (options, arguments, pinned, now): {bad[:3]}"
    # the plane-count rule shows: 95 and 96 planes anisotropic, 111 and 112 isotropic differ by more than a plane's share
    assert len(set(want)) > len(gen.MULTI_PBN) and any(w < 0 for w in want) and any(w > 0 for w in want)


def test_refusals_are_pinned(table):
    want, got = table["refusals"], gen.refusals()
    assert [w[0] for w in want] == [name for name, _ in gen.REFUSALS]
    assert all(w[1] != 0 and w[2] for w in want), "a call of the pinned sweep was not refused"
    bad = [(w, g) for w, g in zip(want, got) if w != g]
    assert not bad, f"{len(bad)} of {len(want)} refusals changed; first (pinned, now): {bad[0]}"
