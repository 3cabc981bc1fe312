"""DARTRAY_STAGE_COUNTS, the diagnostics that read the device counter buffer back BY INDEX (CounterLayout in dr_host.h: the stage
rows, k_env's counts): the figures they print are the stage lists' own lengths, and printing them leaves the film alone -- on a path
render (one round of the stage loop) and on DirectLighting over mirror / glass (several rounds: the round words, the partial reset of
the counters between rounds)."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from dartray_amd import _abi, core, scenes

sys.path.insert(0, GOLDEN)
import make_restatement_fixtures as mrf  # noqa: E402

pytestmark = pytest.mark.gpu

LINE = re.compile(r"^stage_counts batch (\d+) stage (\d+): in (\d+) active_out (\d+) closest (\d+) any (\d+) env (\d+)$", re.M)


def _render_both(r, scene, capfd):
    """The film without the diagnostics, the film with them, and the stage_counts lines of the second render."""
    lib = _abi.lib()
    try:
        _abi.check(lib.dr_set_option(b"STAGE_COUNTS", b""))
        plain = r.render(scene).film
        capfd.readouterr()
        _abi.check(lib.dr_set_option(b"STAGE_COUNTS", b"1"))
        logged = r.render(scene).film
        err = capfd.readouterr().err
    finally:
        _abi.check(lib.dr_set_option(b"STAGE_COUNTS", b""))
    rows = [tuple(int(v) for v in m.groups()) for m in LINE.finditer(err)]
    print(err)
    return plain, logged, rows


def test_stage_counts_of_a_path_render_are_the_stage_lists(gpu, capfd):
    prims, mk = scenes.config("C2", xres=32, yres=32, spp=8, blob=(24, 12))
    r = mk()
    scene = scenes.make_scene(prims)
    plain, logged, rows = _render_both(r, scene, capfd)
    assert np.array_equal(plain, logged)
    st, info = r.last_stats, scene._device().last_render_info()
    n_stages = r.surfaceIntegrator.maxDepth + 2
    slots = 33 * 33 * 8  # the sampler window is one pixel larger than the film; one batch
    assert info["batches"] == 1 and st["camera_samples"] == slots
    assert [(b, s) for b, s, *_ in rows] == [(1, s) for s in range(n_stages)], rows
    prev_out = slots
    for _, stage, n_in, active_out, closest, _any, _env in rows:
        assert n_in == prev_out, (stage, rows)
        assert active_out <= n_in and closest <= 2 * n_in, (stage, rows)
        prev_out = active_out
    print("closest column", [row[4] for row in rows], "camera rays", slots, "closest_rays", st["closest_rays"])
    assert sum(row[4] for row in rows) + slots == st["closest_rays"], (rows, st["closest_rays"])


def test_stage_counts_leave_direct_lighting_over_mirror_and_glass_alone(gpu, capfd):
    """Several rounds of the stage loop per batch (a round per vertex of a slot's ray tree): the recorded serial stream of
    tests/golden/cdlspec_direct_serial.npz through host buffers, with and without the diagnostics."""
    g = np.load(os.path.join(GOLDEN, "cdlspec_direct_serial.npz"))
    prims, mk = mrf.dlspec_case()
    r = mk()
    r.sampler = core.HostBufferSampler(r.camera, 4, g["pixel_xy"], g["sample_vec"])
    plain, logged, rows = _render_both(r, scenes.make_scene(prims), capfd)
    assert np.array_equal(plain, logged)
    assert np.array_equal(logged, g["film"])
    assert len(rows) > 0 and rows[0][2] == 17 * 17 * 4, rows
