"""Generate tests/golden/path_decisions.json: the answer of every path query of the C ABI (admm_query_paths,
admm_query_grouped_paths, admm_query_grouped_path, admm_query_state_path, admm_query_forward_schedule) over a sweep of
calls, the multi-branch workspace sizes on both sides of the plane-count rule (that family has no query: its workspace
layout shows which grid it planned) and the (code, admm_last_error() text) of calls the multi-branch, grouped and state
entry points refuse before any device work (tests/test_capi_path_pins.py compares the library against it).  The table
pins which kernels a call runs and what a wrong call is told: run this from the commit whose decisions are to be kept,
never to make a failing comparison pass.  No GPU needed.

    python tests/golden/gen_path_decisions.py          # rewrites tests/golden/path_decisions.json

The sweep: SHAPES x PROXES x (no PSF, kh = min(M, N, 5)) x PLANES (both sides of every plane-count threshold) x modes
forward / record / backward x rec_flags 0..3 x want_hbar x want_rho, under each option set of OPTION_SETS; the forward
schedule over the planes > 0, and with MALL_STREAMS = 4 at the two shapes and four plane counts of MALL_CASES.
An answer is [forward path, sweep path], [path], [chunk planes, streams], or minus the error code of a refused query.
The file holds the distinct answers once, the distinct run-length encoded answer sequences of a block (family, option
set, shape, prox) once, and per family the sequence index of every block in the order of blocks()."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "admm-deconv_amd"))

from admm_deconv import _lib  # noqa: E402

OUT = os.path.join(HERE, "path_decisions.json")
SHAPES = [(2, 2), (32, 32), (64, 64), (96, 96), (128, 128), (250, 250), (256, 256), (256, 128), (480, 640), (512, 512),
          (37, 29), (1024, 16), (4096, 2)]
PROXES = [False, True, "plane"]
PLANES = [0, 1, 6, 95, 96, 111, 112, 191, 192, 255, 256, 65280]
MODES = [_lib.MODE_FORWARD, _lib.MODE_RECORD, _lib.MODE_BACKWARD]
OPTION_SETS = [{}, {"FUSED": 0}, {"FUSED_ADJ": 0}, {"RESIDENT": 0}, {"RESIDENT": 2}, {"SMOOTH": 0}, {"MIN_PLANES": 0},
               {"MIN_PLANES": 100}]
MALL_CASES = ([(512, 512), (480, 640)], [8, 64, 256, 768])
FAMILIES = ["paths", "grouped_paths", "grouped_path", "state_path", "forward_schedule", "forward_schedule_mall4"]

# multi-branch workspace sizes at 256 x 256: (P, B, nbranch) giving 30, 95, 96, 111, 112 and 960 planes
MULTI_PBN = [(3, 2, 5), (1, 19, 5), (3, 16, 2), (3, 37, 1), (1, 56, 2), (3, 64, 5)]
MULTI_FLAGS = [0, _lib.MULTI_RECORD, _lib.MULTI_RECORD | _lib.REC_MASKS, _lib.MULTI_ISO, _lib.MULTI_RECORD | _lib.MULTI_ISO]
MULTI_MAXITS = [0, 1, 50]
MULTI_OPTION_SETS = [{}, {"MIN_PLANES": 0}, {"MIN_PLANES": 100}, {"FUSED": 0}, {"FUSED_ADJ": 0}]


class options:
    """Every option of the set for the block, restored afterwards."""

    def __init__(self, opts):
        self.cms = [_lib.option(k, v) for k, v in opts.items()]

    def __enter__(self):
        for c in self.cms:
            c.__enter__()

    def __exit__(self, *a):
        for c in reversed(self.cms):
            c.__exit__(*a)


def blocks():
    """(family, option set, (M, N), prox) of every block, in the order of the table's lists."""
    for fam in FAMILIES[:5]:
        for opts in OPTION_SETS:
            for shape in SHAPES:
                for prox in PROXES:
                    yield fam, opts, shape, prox
    for shape in MALL_CASES[0]:
        for prox in PROXES:
            yield "forward_schedule_mall4", {"MALL_STREAMS": 4}, shape, prox


def queries(fam, shape):
    """The argument tuples (kh, planes, mode, flags, want_hbar, want_rho) of a block's queries, in order."""
    for kh in (0, min(shape[0], shape[1], 5)):
        if fam in ("paths", "grouped_paths"):
            for planes in PLANES:
                for mode in MODES:
                    for flags in range(4):
                        for hbar in (0, 1):
                            for rho in (0, 1):
                                yield kh, planes, mode, flags, hbar, rho
        else:
            for planes in (MALL_CASES[1] if fam == "forward_schedule_mall4" else PLANES[1:] if fam == "forward_schedule"
                           else PLANES):
                yield kh, planes, 0, 0, 0, 0


def answers(fam, shape, prox):
    """The answers of a block's queries under the options in force."""
    L = _lib.load()
    M, N = shape
    iso = _lib.iso_code(prox)
    f, b, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_longlong(0)
    pf, pb, pc = ctypes.byref(f), ctypes.byref(b), ctypes.byref(c)
    out = []
    for kh, planes, mode, flags, hbar, rho in queries(fam, shape):
        if fam == "paths":
            rc, a = L.admm_query_paths(M, N, iso, kh, planes, mode, flags, hbar, rho, pf, pb), (f.value, b.value)
        elif fam == "grouped_paths":
            rc = L.admm_query_grouped_paths(M, N, iso, kh, planes, 1, mode, flags, hbar, rho, pf, pb)
            a = (f.value, b.value)
        elif fam == "grouped_path":
            rc, a = L.admm_query_grouped_path(M, N, iso, kh, planes, 1, pf), (f.value,)
        elif fam == "state_path":
            rc, a = L.admm_query_state_path(M, N, iso, kh, planes, pf), (f.value,)
        else:
            rc, a = L.admm_query_forward_schedule(M, N, iso, kh, planes, pc, pf), (c.value, f.value)
        out.append(a if rc == 0 else -abs(rc))
    return out


def rle(seq):
    runs = []
    for a in seq:
        if runs and runs[-1][0] == a:
            runs[-1][1] += 1
        else:
            runs.append([a, 1])
    return runs


def unrle(runs):
    return [a for a, n in runs for _ in range(n)]


def multi_calls():
    for opts in MULTI_OPTION_SETS:
        for P, B, nbr in MULTI_PBN:
            for fl in MULTI_FLAGS:
                for maxit in MULTI_MAXITS:
                    yield opts, (256, 256, P, B, nbr, maxit, fl)


def multi_bytes():
    out = []
    for opts, args in multi_calls():
        with options(opts):
            try:
                out.append(_lib.multi_workspace_bytes(*args))
            except _lib.AdmmError as e:
                out.append(-abs(e.code))
    return out


# ---- refused calls: they fail validation before any device work, so the pointers below are never dereferenced ----
FAKE = 1 << 20        # 256-byte aligned
ODD = FAKE + 4        # not 16-byte aligned
BIG = 1 << 40


def _ptrs(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _fwd_multi(y=FAKE, x=FAKE, M=256, N=256, P=3, B=2, nbr=2, lam="dev", rho="dev", maxit=5, flags=0, ws=FAKE, nbytes=BIG):
    arr = {"dev": _ptrs(*([FAKE] * max(nbr, 1))), None: None, "hole": _ptrs(FAKE, None)}
    return _lib.load().admm_tvd_forward_multi_dev_f32(y, x, M, N, P, B, nbr, arr[lam], arr[rho], maxit, flags, ws, nbytes,
                                                      None)


def _bwd_multi(x_bar=FAKE, y_bar=FAKE, M=256, N=256, P=3, B=2, nbr=2, maxit=5, x_out=FAKE, ws=FAKE, nbytes=BIG):
    return _lib.load().admm_tvd_backward_multi_recorded_dev_f32(x_bar, y_bar, None, None, M, N, P, B, nbr, maxit, x_out, ws,
                                                                nbytes, None)


def _fwd_grouped(y=FAKE, M=64, N=64, P=3, B=5, gb=5, gp=1, h=FAKE, kh=3, lam=FAKE, nparam=5, iso=0, nbytes=BIG, rec=None):
    L = _lib.load()
    if rec is None:
        return L.admm_tvd_forward_grouped_dev_f32(y, FAKE, M, N, P, B, gb, gp, h, kh, kh, lam, FAKE, nparam, iso, 5, FAKE,
                                                  nbytes, None)
    return L.admm_tvd_forward_grouped_record_dev_f32(y, FAKE, M, N, P, B, gb, gp, h, kh, kh, lam, FAKE, nparam, iso, 5, rec,
                                                     FAKE, nbytes, None)


def _bwd_grouped(x_bar=FAKE, y_bar=FAKE, iso=0, nparam=5, ws=FAKE):
    return _lib.load().admm_tvd_backward_grouped_recorded_dev_f32(FAKE, x_bar, y_bar, None, None, None, 64, 64, 3, 5, 5, 1,
                                                                  FAKE, 3, 3, FAKE, FAKE, nparam, iso, 5, FAKE, ws, BIG, None)


def _state(y=FAKE, M=64, N=64, P=3, B=5, h=FAKE, kh=3, lam=FAKE, iso=0, maxit=5, s_in=FAKE, s_out=FAKE + 4096, nbytes=BIG):
    return _lib.load().admm_tvd_forward_state_dev_f32(y, FAKE, M, N, P, B, h, kh, kh, lam, FAKE, iso, maxit, s_in, s_out,
                                                      None, FAKE, nbytes, None)


REFUSALS = [
    ("multi: P = 0", lambda: _fwd_multi(P=0)),
    ("multi: nbranch = 0", lambda: _fwd_multi(nbr=0)),
    ("multi: maxit < 0", lambda: _fwd_multi(maxit=-1)),
    ("multi: unknown flags", lambda: _fwd_multi(flags=8)),
    ("multi: 128 x 256", lambda: _fwd_multi(M=128)),
    ("multi: FUSED = 0", lambda: _with({"FUSED": 0}, _fwd_multi)),
    ("multi: iso recording, FUSED_ADJ = 0",
     lambda: _with({"FUSED_ADJ": 0}, lambda: _fwd_multi(flags=_lib.MULTI_RECORD | _lib.MULTI_ISO))),
    ("multi: too many planes", lambda: _fwd_multi(P=3, B=4353, nbr=5)),
    ("multi: NULL y", lambda: _fwd_multi(y=None)),
    ("multi: NULL x_out", lambda: _fwd_multi(x=None)),
    ("multi: misaligned y", lambda: _fwd_multi(y=ODD)),
    ("multi: misaligned x_out", lambda: _fwd_multi(x=ODD)),
    ("multi: NULL lambda", lambda: _fwd_multi(lam=None)),
    ("multi: NULL rho", lambda: _fwd_multi(rho=None)),
    ("multi: NULL lambda[1]", lambda: _fwd_multi(lam="hole")),
    ("multi: NULL rho[1]", lambda: _fwd_multi(rho="hole")),
    ("multi: NULL workspace", lambda: _fwd_multi(ws=None)),
    ("multi: short workspace", lambda: _fwd_multi(nbytes=16)),
    ("multi: short workspace, 96 planes recording", lambda: _fwd_multi(B=16, flags=_lib.MULTI_RECORD, nbytes=16)),
    ("multi: short workspace, iso", lambda: _fwd_multi(flags=_lib.MULTI_ISO, nbytes=16)),
    ("multi: misaligned workspace", lambda: _fwd_multi(ws=FAKE + 16)),
    ("multi: unknown flags and 128 x 256", lambda: _fwd_multi(flags=8, M=128)),
    ("multi: maxit < 0 and NULL y", lambda: _fwd_multi(maxit=-1, y=None)),
    ("multi: NULL y and NULL lambda", lambda: _fwd_multi(y=None, lam=None)),
    ("multi: NULL lambda[1] and short workspace", lambda: _fwd_multi(lam="hole", nbytes=16)),
    ("multi: misaligned x_out and NULL workspace", lambda: _fwd_multi(x=ODD, ws=None)),
    ("multi replay: B = 0", lambda: _bwd_multi(B=0)),
    ("multi replay: 256 x 128", lambda: _bwd_multi(N=128)),
    ("multi replay: NULL x_bar", lambda: _bwd_multi(x_bar=None)),
    ("multi replay: NULL x_out", lambda: _bwd_multi(x_out=None)),
    ("multi replay: misaligned x_bar", lambda: _bwd_multi(x_bar=ODD)),
    ("multi replay: misaligned y_bar", lambda: _bwd_multi(y_bar=ODD)),
    ("multi replay: no recording", lambda: _bwd_multi(ws=FAKE + 512)),
    ("multi replay: no recording, NULL workspace", lambda: _bwd_multi(ws=None)),
    ("multi replay: 128 x 256 and NULL x_bar", lambda: _bwd_multi(M=128, x_bar=None)),
    ("multi replay: misaligned x_bar and no recording", lambda: _bwd_multi(x_bar=ODD, ws=FAKE + 512)),
    ("grouped: gb = 2 and NULL lambda", lambda: _fwd_grouped(gb=2, lam=None)),
    ("grouped: NULL h and nparam = 2", lambda: _fwd_grouped(h=None, nparam=2)),
    ("grouped: iso with nparam = 5 and NULL y", lambda: _fwd_grouped(iso=1, y=None)),
    ("grouped: NULL y and short workspace", lambda: _fwd_grouped(y=None, nbytes=16)),
    ("grouped record: plane prox and unknown rec_flags", lambda: _fwd_grouped(iso=2, rec=8)),
    ("grouped record: unknown rec_flags and NULL y", lambda: _fwd_grouped(y=None, rec=8)),
    ("grouped replay: misaligned y_bar and NULL x_bar", lambda: _bwd_grouped(y_bar=ODD, x_bar=None)),
    ("grouped replay: no recording", lambda: _bwd_grouped(ws=FAKE + 512)),
    ("state: plane prox and M = 1", lambda: _state(iso=2, M=1)),
    ("state: too many planes and NULL h", lambda: _state(P=256, B=256, h=None)),
    ("state: NULL h and NULL y", lambda: _state(h=None, y=None)),
    ("state: NULL y and maxit = 0", lambda: _state(y=None, maxit=0)),
    ("state: maxit = 0 and state_out = state_in", lambda: _state(maxit=0, s_out=FAKE)),
    ("state: state_out = state_in and misaligned", lambda: _state(s_in=ODD, s_out=ODD)),
    ("state: misaligned state_in and short workspace", lambda: _state(s_in=ODD, nbytes=16)),
    ("state: NULL lambda and M = 1", lambda: _state(lam=None, M=1)),
]


def _with(opts, call):
    with options(opts):
        return call()


def refusals():
    """[[name, code, admm_last_error() text]] of every call of REFUSALS."""
    L = _lib.load()
    out = []
    for name, call in REFUSALS:
        rc = call()
        out.append([name, rc, L.admm_last_error().decode(errors="replace") if rc else ""])
    return out


def measure_blocks():
    """[(block, answers)] in the order of blocks()."""
    out = []
    for fam, opts, shape, prox in blocks():
        with options(opts):
            out.append(((fam, opts, shape, prox), answers(fam, shape, prox)))
    return out


def encode(measured):
    table = {"answers": [], "runs": [], "blocks": {fam: [] for fam in FAMILIES}}
    ai, ri = {}, {}
    for (fam, _, _, _), seq in measured:
        idx = [ai.setdefault(json.dumps(a), len(ai)) for a in seq]
        table["blocks"][fam].append(ri.setdefault(json.dumps(rle(idx)), len(ri)))
    table["answers"] = [json.loads(a) for a in ai]
    table["runs"] = [json.loads(r) for r in ri]
    return table


def decode(table):
    """[answers] per block, in the order of blocks()."""
    it = {fam: iter(v) for fam, v in table["blocks"].items()}
    ans = table["answers"]
    return [[ans[i] for i in unrle(table["runs"][next(it[fam])])] for fam, _, _, _ in blocks()]


if __name__ == "__main__":
    measured = measure_blocks()
    table = encode(measured)
    table["multi_bytes"] = multi_bytes()
    table["refusals"] = refusals()
    with open(OUT, "w") as f:
        json.dump(table, f, separators=(",", ":"))
        f.write("\n")
    print(sum(len(s) for _, s in measured), "queries,", len(table["answers"]), "distinct answers,", len(table["runs"]),
          "distinct blocks,", os.path.getsize(OUT), "bytes")
