"""Reading the committed golden fixtures (tests/golden/*.npz, written by tests/golden/gen_golden.py)."""
import os

import numpy as np


def load(path):
    """The arrays of one fixture as a dict (y, h, x, params).  A fixture whose input and expected output would
    together exceed the repository's limit of 1 MiB per file keeps its input y in tests/golden/inputs/ under the
    same file name."""
    d = dict(np.load(path))   # allow_pickle=False (default)
    if "y" not in d:
        d["y"] = np.load(os.path.join(os.path.dirname(path), "inputs", os.path.basename(path)))["y"]
    return d
