"""Shape "nurbs" on the GPU: dr_nurbs_dice_device writes the bytes dr_nurbs_dice writes (which tests/test_nurbs.py holds
against the restatement of the reference's text) on every patch and dice rate of tests/nurbs_cases.py -- a NaN matching any NaN --, also
with the patch data read from global memory instead of LDS, refuses what it refuses, and a scene with the shape renders like the same
scene with the diced mesh written out."""
import numpy as np
import pytest

from dartray_amd import core, pbrt
from util import rel_err_image

import nurbs_cases as nc
from test_gpu_subdiv import SCENE, _numbers

pytestmark = pytest.mark.gpu


def assert_device_equals_host(kw, du, dv):
    host = core.nurbs_dice(diceu=du, dicev=dv, builder="host", **kw)
    dev = core.nurbs_dice(diceu=du, dicev=dv, builder="device", **kw)
    assert (host[4], dev[4]) == ("host", "device")
    for name, d, h in zip(("P", "N", "uv", "indices"), dev[:4], host[:4]):
        assert nc.same_bits_or_both_nan(d, h), name
    return host


@pytest.mark.parametrize("name", sorted(nc.CASES) + sorted(nc.NAN_CASES))
def test_device_builder_equals_host_builder(gpu, name):
    kw = nc.CASES.get(name) or nc.NAN_CASES[name]
    for du, dv in nc.rates(name):
        assert_device_equals_host(kw, du, dv)


def test_patch_data_too_large_for_lds_is_read_from_global_memory(gpu):
    """40 x 30 control points of order 4 x 3 are 4 877 floats with their knots, above the 4 096 the kernel stages: the other route, the same
    rules, over all 37 x 28 spans."""
    nu, nv = 40, 30
    uk = [0.0] * 4 + [float(i) for i in range(1, nu - 3)] + [float(nu - 3)] * 4
    vk = [0.0] * 3 + [float(i) for i in range(1, nv - 2)] + [float(nv - 2)] * 3
    assert len(uk) + len(vk) + 4 * nu * nv > 4096
    kw = nc._patch(nu, 4, uk, nv, 3, vk, P=nc._net(nu, nv, 6))
    assert_device_equals_host(kw, 65, 3)


@pytest.mark.parametrize("name", sorted(nc.REFUSALS))
def test_device_entry_point_refuses(gpu, name):
    kw, message = nc.REFUSALS[name]
    with pytest.raises(core.DartRayHipError, match="dr_nurbs_dice_device: .*" + message):
        core.nurbs_dice(builder="device", **kw)


def test_nurbs_renders_like_its_diced_mesh_and_like_the_oracle(ob, gpu):
    """One bicubic patch at the default dice rate."""
    from test_nurbs import nurbs_directive
    kw = nc.CASES["bezier_bicubic"]
    P, N, uv, tri, _ = core.nurbs_dice(builder="host", **kw)
    assert not np.isnan(N).any()
    flat = 'Shape "trianglemesh" "integer indices" [%s] "point P" [%s] "normal N" [%s] "float uv" [%s]' % (
        _numbers(tri, "%d"), _numbers(P, "%.9g"), _numbers(N, "%.9g"), _numbers(uv, "%.9g"))
    scene = SCENE.replace("[16]", "[32]")
    a = pbrt.loads(scene.format(shape=nurbs_directive(kw)), render=True)
    b = pbrt.loads(scene.format(shape=flat), render=True)
    mesh = a.scenePrimitives[1].shape
    assert len(mesh.vertexIndex) == 2 * 29 * 29 and mesh.n is not None and mesh.uvs is not None
    assert a.outputImage.film.shape[:2] == (32, 32)
    assert np.array_equal(a.outputImage.film.view(np.uint32), b.outputImage.film.view(np.uint32))
    assert a.outputImage.rgb.mean() > 0.01
    ref = ob.OracleScene(a.scenePrimitives).render(ob.render_desc(a.rendererObject, sampler_mode=1))
    assert rel_err_image(a.outputImage.rgb, ref["rgb"]).max() <= 1e-4
    assert np.array_equal(a.outputImage.film, ref["film"])
