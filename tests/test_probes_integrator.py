"""Radiance probes without a device: the constants and sample slots of DR_INTEGRATOR_USE_PROBES, the value 10 that stays unassigned,
the refusal texts that need no scene, the header / length validation of dr_scene_set_probes, the ProbeGrid text round trip, the Plugin lookup, and
the restatement's own hand-checked known answers."""
import ctypes as C

import numpy as np
import pytest

from dartray_amd import _abi, core

import probes_restatement as pr


def _grid(lmax=1, n=(2, 1, 1), bounds=(0.0, 0.0, 0.0, 2.0, 1.0, 1.0), direct=1.0, seed=3):
    cells, terms = n[0] * n[1] * n[2], (lmax + 1) ** 2
    rng = np.random.RandomState(seed)
    coeff = rng.uniform(-1.0, 1.0, cells * terms * 3) * 10.0 ** rng.randint(-12, 6, cells * terms * 3)
    return np.concatenate([[lmax, direct, 0.0], n, bounds, coeff, [0.0, 0.0, 0.0]]).astype(np.float32)


def test_the_restatements_known_answers():
    assert pr.known_answers()


def test_constant_and_sample_slots():
    lib = _abi.lib()
    assert _abi.DR_INTEGRATOR_USE_PROBES == 11 and core.UseProbesIntegrator.kind == 11
    for nl in (0, 1, 3):   # requestSamples asks for DirectLighting "all"'s slots (use_probes_integrator.dart:74-88)
        assert lib.dr_sample_floats(11, nl) == lib.dr_sample_floats(_abi.DR_INTEGRATOR_DIRECT_ALL, nl) == 5 + 2 * nl + 2 + 2 * 2 * nl
    # 10 stays unassigned, as 6 and 8 do: answered as every unknown value is
    assert lib.dr_sample_floats(10, 3) == lib.dr_sample_floats(6, 3) == lib.dr_sample_floats(8, 3) == lib.dr_sample_floats(12, 3) == lib.dr_sample_floats(99, 3) == 25
    # ... and the integrators around it keep their own slots (tau + scatter only)
    assert lib.dr_sample_floats(_abi.DR_INTEGRATOR_GLOSSY_PRT, 3) == 7
    assert lib.dr_abi_version() == 9


def test_request_samples_are_the_direct_lighting_all_slots():
    class _L:
        def __init__(self, n):
            self.nSamples = n

    class _S:
        lights = [_L(1), _L(4), _L(3)]

    class _Sampler:
        roundSize = staticmethod(core.RoundUpPow2)
    a = core.UseProbesIntegrator().requestSamples(_Sampler, _S)
    b = core.DirectLightingIntegrator().requestSamples(_Sampler, _S)
    assert a == b == ([1, 1, 4, 4, 4, 4], [1, 1, 4, 4, 4, 4])


def test_plugin_lookup_and_the_adaptive_refusal():
    core.RegisterStandardPlugins()
    create = core.Plugin.get("surfaceIntegrator", "useprobes")
    assert create is core.UseProbesIntegrator.Create
    with pytest.raises(ValueError, match="use probes: cannot read the probe file .*`filename` parameter"):
        create({"filename": "no/such/probes.out"})
    with pytest.raises(ValueError, match="use probes: the adaptive sampler is not supported"):
        core.UseProbesIntegrator(_grid()).check_sampler(core.AdaptiveSampler.__new__(core.AdaptiveSampler))


def _set(data):
    lib = _abi.lib()
    a = np.ascontiguousarray(data, np.float32)
    return lib.dr_scene_set_probes(None, a.ctypes.data, len(a)), lib.dr_last_error().decode()


def test_set_probes_validates_the_header_against_the_length():
    good = _grid()
    assert _set(good) == (-1, "null argument")           # a sound grid gets as far as the missing scene
    assert "at least 15 floats" in _set(good[:14])[1]
    for lmax in (0, 9, -3):
        bad = good.copy()
        bad[0] = lmax
        rc, why = _set(bad)
        assert rc == -1 and "use probes: lmax of the grid is outside 1 .. 8" in why
    for k, v in ((3, 0.0), (4, 2.5), (5, 5000.0), (3, -1.0)):
        bad = good.copy()
        bad[k] = v
        assert "nProbes of the grid must be whole numbers in 1 .. 4096" in _set(bad)[1]
    for bad in (good[:-1], np.append(good, 0.0), _grid(lmax=2)[:len(good)]):
        rc, why = _set(bad)
        assert rc == -1 and "the grid's length is not 15 + nProbes[0] * nProbes[1] * nProbes[2] * (lmax + 1)^2 * 3" in why
    bad = good.copy()
    bad[7] = np.inf
    assert "not finite" in _set(bad)[1]
    for lmax, n in ((8, (1, 1, 1)), (2, (3, 2, 2))):
        assert _set(_grid(lmax, n)) == (-1, "null argument")


def test_the_bake_refuses_indirect_lighting_and_lmax_by_name():
    lib = _abi.lib()
    d = _abi.DrProbesDesc()
    d.lmax, d.include_indirect, d.npoints, d.spacing = 4, 1, 96, 1.0
    assert lib.dr_probes_bake(None, C.byref(d), None, 0) == -4
    assert "create probes: indirectlighting is not supported" in lib.dr_last_error().decode()
    for lmax in (0, 9):
        d.lmax, d.include_indirect = lmax, 0
        assert lib.dr_probes_bake(None, C.byref(d), None, 0) == -1
        assert "create probes: lmax must be in 1 .. 8" in lib.dr_last_error().decode()
    # the Python default is explicit about the difference to the reference's default (true)
    import inspect
    assert inspect.signature(core.SamplerRenderer.create_probes).parameters["indirectlighting"].default is False
    assert inspect.signature(core.SamplerRenderer.create_probes).parameters["npoints"].default == 32768


def test_probe_grid_text_round_trip_is_bit_exact(tmp_path):
    g = core.ProbeGrid(_grid(2, (2, 2, 1), seed=11))
    assert g.lmax == 2 and g.nProbes == (2, 2, 1) and g.includeDirect == 1 and g.includeIndirect == 0 and g.coefficients.shape == (4, 9, 3)
    path = str(tmp_path / "probes.out")
    g.save(path)
    back = core.ProbeGrid.load(path)
    assert np.array_equal(back.data.view(np.uint32), g.data.view(np.uint32))
    # the text is what ReadFloatFile reads (common.dart:188-236): comments from '#', numbers of digits . e - + only, and a newline behind the last
    text = open(path).read()
    body = "".join(line.split("#", 1)[0] + "\n" for line in text.splitlines())
    assert text.endswith("\n") and set(body) <= set("0123456789.e-+ \n")
    assert isinstance(core.UseProbesIntegrator(path).probes, core.ProbeGrid)
    with pytest.raises(ValueError, match="not finite"):
        bad = g.data.copy()
        bad[20] = np.nan
        core.ProbeGrid(bad).save(path)


def test_the_descriptor_matches_the_header():
    assert C.sizeof(_abi.DrProbesDesc) == 72
    assert _abi.DrProbesDesc.bounds.offset == 16 and _abi.DrProbesDesc.camera_pos.offset == 40 and _abi.DrProbesDesc.spacing.offset == 56 and _abi.DrProbesDesc.time.offset == 64
