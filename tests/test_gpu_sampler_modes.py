"""Every sampler mode of the device against a frozen picture of itself (tests/golden/sampler_modes.npz, written once by
tests/golden/make_sampler_mode_goldens.py, which also defines the entries): film, image, dr_scene_last_render_info, the sample counts, the
sampler's dump and the supersampled pixels bit for bit, per mode and integrator on C1 at 16 x 12; two two-batch renders at 40 x 32 (at 40 x 24 the one-batch slack of planBatches still makes one batch); and the
(return code, message) pair of every refused descriptor as text.  What the planner decides per mode may be reorganised; what it decides may not.

Halton films are the one exception to bit equality: samples are not grouped by pixel, the order of a pixel's atomic additions is free
(tests/test_gpu_halton.py).  Their weight channel and dumps are compared bit for bit, X / Y / Z within the stored bound (2 n + 4) 2^-24 S
(film_reference.bound of the oracle's radiances), as test_two_batches_equal_one compares its two renders."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import make_sampler_mode_goldens as mg  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "sampler_modes.npz"))


def _stored(golden, entry):
    keys = [k for k in golden.files if k.startswith(entry + "/")]
    assert keys, entry
    return {k[len(entry) + 1:]: golden[k] for k in keys}


def _equal(got, want, entry):
    """Every stored field of the entry, bit for bit (film_bound belongs to a Halton film: see _halton_film)."""
    assert set(got) == set(want) - {"film_bound"}, (entry, sorted(got), sorted(want))
    for k, v in got.items():
        assert np.asarray(v).dtype == want[k].dtype and np.asarray(v).shape == want[k].shape, (entry, k)
        assert np.array_equal(np.asarray(v).view(np.uint32) if want[k].dtype == np.float32 else v,
                              want[k].view(np.uint32) if want[k].dtype == np.float32 else want[k]), (entry, k)


@pytest.mark.parametrize("mode", [m for m in mg.MODES if m[0] != "halton"], ids=mg.mode_key)
def test_mode_equals_its_golden(gpu, golden, mode):
    _equal(mg.mode_entry(*mode), _stored(golden, mg.mode_key(mode)), mg.mode_key(mode))


@pytest.mark.parametrize("mode", [m for m in mg.MODES if m[0] == "halton"], ids=mg.mode_key)
def test_halton_mode_equals_its_golden(gpu, golden, mode):
    got, want = mg.mode_entry(*mode), _stored(golden, mg.mode_key(mode))
    film, gfilm = got.pop("film"), want.pop("film")
    _equal(got, want, mg.mode_key(mode))
    assert np.array_equal(film[..., 3], gfilm[..., 3])
    err = np.abs(film.astype(np.float64) - gfilm.astype(np.float64))
    print("max |film - golden| / bound = %.3g" % float((err[..., :3] / np.maximum(want["film_bound"][..., :3], 1e-300)).max()))
    assert (err <= want["film_bound"]).all()
    assert np.isfinite(film).all() and film[..., :3].max() > 0


def test_host_buffer_replay_equals_its_golden(ob, gpu, golden):
    _equal(mg.host_buffer_entry(ob), _stored(golden, "hostbuf-path"), "hostbuf-path")


@pytest.mark.parametrize("which", mg.TWO_BATCH)
def test_two_batches_equal_their_golden(gpu, golden, which):
    got, want = mg.two_batch_entry(which), _stored(golden, which)
    assert got["counts"][2] == 2 and got["info"][5] == 2
    assert got["info"][7] == want["info"][7]  # overlap, coherent camera, lazy generation
    assert np.array_equal(got["film"].view(np.uint32), want["film"].view(np.uint32))


@pytest.mark.parametrize("name", mg.REFUSALS)
def test_refusal_text_and_code(gpu, golden, name):
    assert mg.refusal(name) == str(golden["refusal/" + name][()])
