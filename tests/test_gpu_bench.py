"""A plain bench.py run on the GPU (no --full): it times exactly --steps steps, prints the headline without the
measurements --full adds, and --dump-outputs writes the image and film of its last step -- the same film and image
as a render of the same scene through SamplerRenderer.render."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_times_its_steps_and_dumps_the_last_one(gpu, tmp_path):
    from dartray_amd import scenes
    out = tmp_path / "outputs"
    env = dict(os.environ, DARTRAY_BENCH_DETAIL_DIR=str(tmp_path))
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--res", "64", "--spp", "4", "--blob", "40,20", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(64 * 64 * 4 / line["ms_per_step"] / 1e3, rel=1e-2)
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert k in line, k
    for k in ("cpu_baseline", "cpu_baseline_threads", "replay_Msamples_s", "extra_configs", "roofline_others"):
        assert k not in line, k
    assert line["roofline"] is None
    rgb, film = np.load(out / "rgb.npy"), np.load(out / "film.npy")
    assert rgb.dtype == film.dtype == np.float32 and rgb.shape == (64, 64, 3) and film.shape == (64, 64, 4)
    prims, mk = scenes.config("C2", xres=64, yres=64, spp=4, blob=(40, 20))
    want = mk().render(scenes.make_scene(prims))
    assert np.array_equal(film, want.film) and np.array_equal(rgb, want.rgb)
