"""Shape "loopsubdiv" on the CPU: the host builder dr_loop_subdivide against tests/loop_restatement.py -- the reference's
text restated in its own pointer style -- bit for bit on P, N and indices; the counts; every refusal by its message; the PBRT front end."""
import numpy as np
import pytest

from dartray_amd import core, pbrt

import loop_restatement
from loop_meshes import LEVELS, MESHES, REFUSALS, euler_counts, fuzz_case

_RESTATED = {}


def restated(key, idx, P, nlevels):
    """The restatement's (P, N, indices), computed once per case and left unchanged."""
    if key not in _RESTATED:
        out = loop_restatement.refine(idx, P, nlevels)
        for a in out:
            a.setflags(write=False)
        _RESTATED[key] = out
    return _RESTATED[key]


def assert_same_bits(got, want):
    for name, g, w in zip(("P", "N", "indices"), got, want):
        assert g.shape == w.shape, name
        assert np.array_equal(np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32)), name


@pytest.mark.parametrize("nlevels", LEVELS)
@pytest.mark.parametrize("name", sorted(MESHES))
def test_host_builder_equals_the_restatement(hip, name, nlevels):
    idx, P = MESHES[name]
    got = core.loop_subdivide(idx, P, nlevels, builder="host")
    assert got[3] == "host"
    want = restated((name, nlevels), idx, P, nlevels)
    assert_same_bits(got[:3], want)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert np.abs(got[1]).max() > 0.0


@pytest.mark.parametrize("nlevels", LEVELS)
@pytest.mark.parametrize("name", sorted(MESHES))
def test_counts(hip, name, nlevels):
    """nf * 4^L faces and, by Euler's relation, the vertices -- from the size query alone and from the full call."""
    import ctypes as C
    idx, P = MESHES[name]
    nf, nv = euler_counts(idx, nlevels)
    assert nf == len(idx) * 4 ** nlevels
    qv, qf = C.c_uint64(0), C.c_uint64(0)
    hip.check(hip.lib().dr_loop_subdivide(idx.ctypes.data, len(idx), P.ctypes.data, len(P), nlevels, None, None, None, 0, 0, C.byref(qv), C.byref(qf)))
    assert (qf.value, qv.value) == (nf, nv)
    Pout, N, iout, _ = core.loop_subdivide(idx, P, nlevels, builder="host")
    assert (len(iout), len(Pout), len(N)) == (nf, nv, nv)
    assert int(iout.max()) == nv - 1 and len(np.unique(iout)) == nv
    edges = {tuple(sorted((int(f[k]), int(f[(k + 1) % 3])))) for f in iout for k in range(3)}
    euler0 = len(P) - len({tuple(sorted((int(f[k]), int(f[(k + 1) % 3])))) for f in idx for k in range(3)}) + len(idx)
    assert nv - len(edges) + nf == euler0


def test_too_small_buffers_are_refused(hip):
    import ctypes as C
    idx, P = MESHES["quad"]
    out = np.zeros((9, 3), np.float32)
    tri = np.zeros((8, 3), np.uint32)
    qv, qf = C.c_uint64(0), C.c_uint64(0)
    rc = hip.lib().dr_loop_subdivide(idx.ctypes.data, len(idx), P.ctypes.data, len(P), 1, out.ctypes.data, out.ctypes.data, tri.ctypes.data,
                                     8, 8, C.byref(qv), C.byref(qf))
    assert rc == -1 and b"too small" in hip.lib().dr_last_error()
    assert (qv.value, qf.value) == (9, 8)


def test_fuzz_permuted_rotated_jittered(hip):
    """20 seeded cases: face order permuted, every face rotated, positions jittered.  Equality with the restatement must hold; and the
    permutation must reach the bits (startFace and the ring order decide every sum), or the test would not be exercising them."""
    differs = 0
    for seed in range(20):
        name, idx, P = fuzz_case(seed)
        nlevels = 1 + seed % 2
        got = core.loop_subdivide(idx, P, nlevels, builder="host")
        assert_same_bits(got[:3], restated(("fuzz", seed), idx, P, nlevels))
        # the unpermuted mesh with the same jittered positions: the same surface, numbered and summed differently
        plain = core.loop_subdivide(MESHES[name][0], P, nlevels, builder="host")
        a = np.sort(got[0].view(np.uint32).reshape(-1, 3).view([("", np.uint32)] * 3).reshape(-1))
        b = np.sort(plain[0].view(np.uint32).reshape(-1, 3).view([("", np.uint32)] * 3).reshape(-1))
        differs += int(not np.array_equal(a, b))
    assert differs >= 1


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(hip, name):
    idx, P, nlevels, message = REFUSALS[name]
    with pytest.raises(core.DartRayHipError, match=message):
        core.loop_subdivide(idx, P, nlevels, builder="host")


LOOP = '''
LookAt 0 0 -8  0 0 0  0 1 0
Camera "perspective" "float fov" [40]
WorldBegin
AttributeBegin
  Translate 0.5 -0.25 1  Rotate 25 0 1 0  Scale 1.5 1 0.75
  Material "matte" "color Kd" [0.6 0.5 0.4]
  Shape "loopsubdiv" "integer nlevels" [2] "integer indices" [{indices}] {points}
AttributeEnd
WorldEnd
'''


def _directive(points=True):
    idx, P = MESHES["icosahedron"]
    pts = '"point P" [%s]' % " ".join("%.9g" % c for c in P.reshape(-1)) if points else ""
    return LOOP.format(indices=" ".join(str(int(i)) for i in idx.reshape(-1)), points=pts)


def test_loader_refines_loopsubdiv_under_a_transform(hip):
    api = pbrt.loads(_directive())
    assert len(api.scenePrimitives) == 1
    mesh = api.scenePrimitives[0].shape
    assert isinstance(mesh, core.TriangleMesh) and isinstance(api.scenePrimitives[0].material, core.MatteMaterial)
    idx, P = MESHES["icosahedron"]
    Pl, N, tri, _ = core.loop_subdivide(idx, P, 2, builder="host")
    assert not np.array_equal(mesh.objectToWorld, np.eye(4, dtype=np.float32))
    assert np.array_equal(mesh.vertexIndex, tri)
    assert np.array_equal(mesh.P.view(np.uint32), core.transform_points(mesh.objectToWorld, Pl).view(np.uint32))
    assert np.array_equal(mesh.n.view(np.uint32), N.view(np.uint32))    # object space, with the transform beside them
    assert not np.array_equal(mesh.P, Pl)
    shape = core.LoopSubdivision(mesh.objectToWorld, mesh.worldToObject, False, idx, P, 2)
    again = shape.refine(builder="host")
    assert shape.builder == "host" and not shape.canIntersect()
    assert np.array_equal(again.P.view(np.uint32), mesh.P.view(np.uint32))
    lo, hi = shape.worldBound()
    assert (lo <= core.transform_points(mesh.objectToWorld, P)).all() and (hi >= core.transform_points(mesh.objectToWorld, P)).all()


def test_loader_drops_loopsubdiv_without_P(hip):
    api = pbrt.loads(_directive(points=False))
    assert api.scenePrimitives == []


def test_loader_default_nlevels_is_one(hip):
    api = pbrt.loads(_directive().replace('"integer nlevels" [2] ', ""))
    assert len(api.scenePrimitives[0].shape.vertexIndex) == 80
