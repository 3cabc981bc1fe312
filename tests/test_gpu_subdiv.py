"""Shape "loopsubdiv" on the GPU: dr_loop_subdivide_device writes the bytes dr_loop_subdivide writes (which
tests/test_loop_subdivision.py holds against the restatement of the reference's text), refuses what it refuses, and a scene with the shape
renders like the same scene with the refined mesh written out."""
import numpy as np
import pytest

from dartray_amd import core, pbrt
from util import rel_err_image

from loop_meshes import LEVELS, MESHES, REFUSALS, fuzz_case, grid

pytestmark = pytest.mark.gpu


def assert_device_equals_host(idx, P, nlevels):
    host = core.loop_subdivide(idx, P, nlevels, builder="host")
    dev = core.loop_subdivide(idx, P, nlevels, builder="device")
    assert (host[3], dev[3]) == ("host", "device")
    for name, d, h in zip(("P", "N", "indices"), dev[:3], host[:3]):
        assert d.shape == h.shape, name
        assert np.array_equal(d.view(np.uint32), h.view(np.uint32)), name
    return host


@pytest.mark.parametrize("name", sorted(MESHES))
def test_device_builder_equals_host_builder(gpu, name):
    for nlevels in LEVELS:
        assert_device_equals_host(*MESHES[name], nlevels)


def test_several_workgroups_of_edge_slots(gpu):
    """6 x 6 vertices, 50 faces, nlevels 4: the last two levels number 2 400 and 9 600 edge slots -- 9.4 and 37.5 workgroups of 256, so
    the block sums, the scan over them and a ragged last workgroup all take part (neither count is a multiple of 256 or 1024)."""
    idx, P = grid(6)
    assert len(idx) == 50 and (3 * 50 * 16) % 256 != 0 and (3 * 50 * 64) % 256 != 0
    host = assert_device_equals_host(idx, P, 4)
    assert len(host[2]) == 12800


@pytest.mark.parametrize("seed", range(5))
def test_device_builder_on_fuzz_cases(gpu, seed):
    _, idx, P = fuzz_case(seed)
    assert_device_equals_host(idx, P, 1 + seed % 2)


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_device_entry_point_refuses(gpu, name):
    idx, P, nlevels, message = REFUSALS[name]
    with pytest.raises(core.DartRayHipError, match="dr_loop_subdivide_device: .*" + message):
        core.loop_subdivide(idx, P, nlevels, builder="device")


SCENE = '''
Film "image" "integer xresolution" [16] "integer yresolution" [16]
SurfaceIntegrator "path" "integer maxdepth" [3]
Sampler "lowdiscrepancy" "integer pixelsamples" [4]
LookAt 0 1 -9  0 0 0  0 1 0
Camera "perspective" "float fov" [35]
WorldBegin
AttributeBegin
  AreaLightSource "area" "color L" [20 19 17] "integer nsamples" [1]
  Translate 0 6 -2
  Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-3 0 -3  3 0 -3  3 0 3  -3 0 3]
AttributeEnd
AttributeBegin
  Material "matte" "color Kd" [0.7 0.6 0.5]
  Translate 0.2 -0.1 0  Rotate 20 0 1 0  Scale 1.2 1 1
  {shape}
AttributeEnd
WorldEnd
'''


def _numbers(a, fmt):
    return " ".join(fmt % c for c in np.asarray(a).reshape(-1))


def test_loopsubdiv_renders_like_its_refined_mesh_and_like_the_oracle(ob, gpu):
    idx, P = MESHES["icosahedron"]
    loop = 'Shape "loopsubdiv" "integer nlevels" [2] "integer indices" [%s] "point P" [%s]' % (_numbers(idx, "%d"), _numbers(P, "%.9g"))
    Pl, N, tri, _ = core.loop_subdivide(idx, P, 2, builder="host")
    flat = 'Shape "trianglemesh" "integer indices" [%s] "point P" [%s] "normal N" [%s]' % (_numbers(tri, "%d"), _numbers(Pl, "%.9g"),
                                                                                        _numbers(N, "%.9g"))
    a = pbrt.loads(SCENE.format(shape=loop), render=True)
    b = pbrt.loads(SCENE.format(shape=flat), render=True)
    assert len(a.scenePrimitives[1].shape.vertexIndex) == 320 and a.scenePrimitives[1].shape.n is not None
    assert np.array_equal(a.outputImage.film.view(np.uint32), b.outputImage.film.view(np.uint32))
    assert a.outputImage.rgb.mean() > 0.01
    ref = ob.OracleScene(a.scenePrimitives).render(ob.render_desc(a.rendererObject, sampler_mode=1))
    assert rel_err_image(a.outputImage.rgb, ref["rgb"]).max() <= 1e-4
    assert np.array_equal(a.outputImage.film, ref["film"])
