"""What the host classes write into the C ABI's descriptors, checked on the CPU against tests/golden/descriptors.json -- recorded by
tests/golden/make_descriptor_goldens.py from the single-file core.py, whose _DeviceScene.__init__ and SamplerRenderer.describe
marshalled every class themselves.  Here the same canonical forms come from describe_scene and SamplerRenderer.describe, which
need no device."""
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_descriptor_goldens as mdg  # noqa: E402

import dartray_amd  # noqa: E402
from dartray_amd import core  # noqa: E402

RECORDED = json.load(open(os.path.join(GOLDEN, "descriptors.json")))


@pytest.fixture(autouse=True)
def host_builder(monkeypatch):
    """The goldens were built by the host builders; a process that has selected a GPU would pick the device's."""
    monkeypatch.setenv("DARTRAY_BVH_BUILDER", "host")


def _mismatches(got, want, what):
    return ["%s: %s" % (what, k) for k in sorted(set(got) | set(want)) if got.get(k) != want.get(k)]


def test_descriptors_equal_the_recorded_ones():
    bad, seen = [], set()
    for name, make in mdg.scene_cases().items():
        for i, scene in enumerate(make()):
            key = "%s/%d" % (name, i)
            seen.add(key)
            d, keep, general = core.describe_scene(scene.aggregate, scene.lights)
            bad += _mismatches(mdg.canonical(d), RECORDED["scenes"][key], "scene " + key)
            if general != RECORDED["general"][key]:
                bad.append("scene %s: general" % key)
    assert seen == set(RECORDED["scenes"]) == set(RECORDED["general"])
    renders = mdg.render_cases()
    assert set(renders) == set(RECORDED["renders"])
    for name, make in renders.items():
        d, keep = make().describe()
        bad += _mismatches(mdg.canonical(d), RECORDED["renders"][name], "render " + name)
    assert not bad, bad


def test_describe_scene_needs_no_device(monkeypatch):
    """describe_scene is host work: it neither selects a device nor asks for the library."""
    from dartray_amd import _abi
    scene = mdg.scene_cases()["mixed"]()[0]

    def refuse(*a, **k):
        raise AssertionError("describe_scene touched the library")
    monkeypatch.setattr(_abi, "init", refuse)
    monkeypatch.setattr(_abi, "lib", refuse)
    d, keep, general = core.describe_scene(scene.aggregate, scene.lights)
    assert d.nlights == len(scene.lights) and general


def test_every_recorded_name_is_still_there():
    missing = [n for n in RECORDED["names"]["core"] if not hasattr(core, n)]
    assert not missing, missing
    assert mdg.public_names() == RECORDED["names"]["dartray_amd"]
    scope = {}
    exec("from dartray_amd import *", scope)
    assert set(RECORDED["names"]["dartray_amd"]) <= set(scope) and hasattr(dartray_amd, "core")


def test_error_paths_raise_on_the_host():
    prims = mdg.scenes.cornell_c1_prims()
    accel = core.BVHAccel(prims, builder="host")
    with pytest.raises(ValueError, match="an emissive primitive's area light is missing from Scene.lights"):
        core.describe_scene(accel, [])
    with pytest.raises(ValueError, match="an emissive primitive's area light is missing from Scene.lights"):
        core.Scene(accel, [core.PointLight()])._device()
    with pytest.raises(ValueError, match="builder must be 'device' or 'host'"):
        core.BVHAccel(prims, builder="gpu")
    with pytest.raises(ValueError, match="builder must be 'device' or 'host'"):
        core.loop_subdivide([0, 1, 2], [[0, 0, 0], [1, 0, 0], [0, 1, 0]], 1, builder="gpu")
