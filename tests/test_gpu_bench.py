"""GPU: a plain `bench.py --gpus 1 --steps N --warmup W` run times its steps and nothing else, and
--dump-outputs writes the batch its last timed step solved (here a small batch, under the library's own
plane-count rule as in the benchmark process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import admm_deconv
from admm_deconv import synth
from conftest import REPO

pytestmark = pytest.mark.gpu


@pytest.mark.min_planes_rule
def test_plain_run_is_lean_and_dumps_the_solved_batch(dev, tmp_path):
    B, distinct = 6, 4
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--batch", str(B), "--distinct", str(distinct), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, env=env, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["unit"] == "images/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["ms_per_step"] > 0
    # value and ms_per_step are the same measurement (both rounded in the line)
    assert d["value"] == pytest.approx(B * 1000.0 / d["ms_per_step"], rel=1e-3)
    # what --full adds is not measured in a plain run
    for k in ("roofline", "kernels", "cpu_baseline", "ranks", "solve_only"):
        assert k not in d
    assert os.listdir(out) == ["x.npy"]
    x = np.load(out / "x.npy")
    cfg = synth.CONFIGS["c2"]
    assert x.dtype == np.float32 and x.shape == (B, cfg["P"], cfg["N"], cfg["M"])
    # the same seeded inputs through the same library call in this process: the same planes, bit for bit
    psf = synth.gaussian_psf(*cfg["psf"])
    base = synth.make_batch(distinct, cfg["M"], cfg["N"], psf, P=cfg["P"])
    y = np.ascontiguousarray(np.concatenate([base, base])[:B])
    ref = admm_deconv.tvd_fft(torch.from_numpy(y).to(dev), synth.LAMBDA, synth.RHO, torch.from_numpy(psf).to(dev),
                              False, cfg["K"])
    torch.cuda.synchronize()
    assert np.array_equal(x, ref.cpu().numpy())
