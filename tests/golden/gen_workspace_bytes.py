"""Generate tests/golden/workspace_bytes.json: the byte count every workspace size query of the C ABI returns over a
sweep of calls (tests/test_capi_workspace_pins.py compares the library against it).  The table pins the workspace
layouts: run this from the commit whose layouts are to be kept, never to make a failing comparison pass.  No GPU needed.

    python tests/golden/gen_workspace_bytes.py          # rewrites tests/golden/workspace_bytes.json

The sweep: the shapes of tests/asan/capi_host_check.c at P = 3, B = 5, crossed with both proxes, no PSF / 1 x 1 /
15 x 10 (clipped to the image), every grouping (gb, gp) in {1, B} x {1, P}, maxit 0 / 1 / 7 and the recording flags
0 / HBAR / MASKS; the multi-branch query at 256 x 256 with 2 branches and its five flag words."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "admm-deconv_amd"))

from admm_deconv import _lib  # noqa: E402

OUT = os.path.join(HERE, "workspace_bytes.json")
SHAPES = [(2, 2), (3, 5), (64, 64), (96, 96), (250, 250), (256, 256), (480, 640), (512, 512), (37, 29), (1024, 16),
          (2048, 2048), (4096, 2)]
P, B, NBRANCH = 3, 5, 2
GROUPINGS = [(1, 1), (B, 1), (1, P), (B, P)]
MAXITS = [0, 1, 7]
REC_FLAGS = [0, _lib.REC_HBAR, _lib.REC_MASKS]
MULTI_FLAGS = [0, _lib.MULTI_RECORD, _lib.MULTI_RECORD | _lib.REC_MASKS, _lib.MULTI_ISO, _lib.MULTI_RECORD | _lib.MULTI_ISO]
QUERIES = {
    "forward": _lib.workspace_bytes,
    "backward": _lib.backward_workspace_bytes,
    "grouped": _lib.grouped_workspace_bytes,
    "grouped_backward": _lib.grouped_backward_workspace_bytes,
    "multi": _lib.multi_workspace_bytes,
}


def calls():
    """(query name, arguments) of every pinned call, in the order of the table's lists."""
    for M, N in SHAPES:
        for iso in (0, 1):
            for kh, kw in ((0, 0), (1, 1), (min(M, 15), min(N, 10))):
                yield "forward", (M, N, P, B, kh, kw, iso)
                for maxit in MAXITS:
                    for fl in REC_FLAGS:
                        yield "backward", (M, N, P, B, kh, kw, iso, maxit, fl)
                for gb, gp in GROUPINGS:
                    yield "grouped", (M, N, P, B, gb, gp, kh, kw, iso)
                    for maxit in MAXITS:
                        for fl in REC_FLAGS:
                            yield "grouped_backward", (M, N, P, B, gb, gp, kh, kw, iso, maxit, fl)
    for fl in MULTI_FLAGS:
        for maxit in MAXITS:
            yield "multi", (256, 256, P, B, NBRANCH, maxit, fl)


def measure():
    """{query name: [bytes, or minus the error code of a refused query, per call of calls()]}"""
    table = {name: [] for name in QUERIES}
    for name, args in calls():
        try:
            table[name].append(QUERIES[name](*args))
        except _lib.AdmmError as e:
            table[name].append(-abs(e.code))
    return table


if __name__ == "__main__":
    table = measure()
    with open(OUT, "w") as f:
        json.dump(table, f, separators=(",", ":"))
        f.write("\n")
    print({k: len(v) for k, v in table.items()}, os.path.getsize(OUT), "bytes")
