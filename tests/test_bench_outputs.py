"""bench.py --dump-outputs and --full, without a GPU: what the dump writes (float arrays by name, at most 64 MB, the same
fixed pixel sample from run to run above that), and that the command line knows both options."""
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _images(h, w):
    rng = np.random.default_rng(7)
    return {"rgb": rng.random((h, w, 3), dtype=np.float32), "film": rng.random((h, w, 4), dtype=np.float32)}


def test_dump_writes_every_image_whole_under_the_limit(tmp_path):
    img = _images(48, 64)
    bench.dump_outputs(str(tmp_path / "out"), img)
    for name, v in img.items():
        got = np.load(tmp_path / "out" / (name + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, v), name


def test_dump_casts_to_float32(tmp_path):
    img = {"rgb": np.arange(2 * 3 * 3, dtype=np.float16).reshape(2, 3, 3)}
    bench.dump_outputs(str(tmp_path), img)
    got = np.load(tmp_path / "rgb.npy")
    assert got.dtype == np.float32 and np.array_equal(got, img["rgb"].astype(np.float32))


def test_dump_above_the_limit_is_the_same_pixel_sample_of_every_image(tmp_path):
    img = _images(256, 256)  # 1.8 MB
    limit = 1 << 20
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), img, limit=limit)
    total = sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) for n in img)
    assert total <= limit
    rgb, film = (np.load(tmp_path / "a" / (n + ".npy")) for n in ("rgb", "film"))
    assert rgb.shape[1] == 3 and film.shape[1] == 4 and len(rgb) == len(film) > 0.5 * limit / 28
    for n in img:  # the sample does not change from run to run
        assert np.array_equal(np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy")))
    # the rows are pixels of the image, in pixel order, and the two files hold the same pixels
    flat_rgb, flat_film = img["rgb"].reshape(-1, 3), img["film"].reshape(-1, 4)
    where = {tuple(v): i for i, v in enumerate(flat_rgb)}
    idx = np.array([where[tuple(v)] for v in rgb])
    assert np.all(np.diff(idx) > 0) and np.array_equal(flat_film[idx], film)


def test_the_command_line_has_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout
