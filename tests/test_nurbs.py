"""Shape "nurbs" on the CPU: the host builder dr_nurbs_dice against tests/nurbs_restatement.py -- the reference's text
(shapes/nurbs.dart:76-263) restated line by line -- byte for byte on the patches of tests/nurbs_cases.py; the index list; the known
answers; every refusal by name; the size query and the capacity check; core.Nurbs' bounds; the loader; the three places that name the
entry points; and the host code under the address and undefined-behaviour sanitizers as a stand-alone program.

The builders and the restatement repair two index expressions of the reference's text;
test_the_text_as_it_stands_raises_and_leaves_the_surface shows on the unrepaired restatement what those two lines do."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dartray_amd import _abi, core, pbrt

import nurbs_cases as nc

ALL = list(nc.every_case())
DR_ERR_INVALID = -1  # include/dartray_hip.h
IDS = ["%s-%dx%d" % (name, du, dv) for name, _, du, dv in ALL]


def dice(kw, du=30, dv=30, builder="host"):
    return core.nurbs_dice(diceu=du, dicev=dv, builder=builder, **kw)


@pytest.mark.parametrize("name,kw,du,dv", ALL, ids=IDS)
def test_host_builder_equals_the_restatement(name, kw, du, dv):
    got = dice(kw, du, dv)
    ref = nc.restated(name, du, dv)
    assert got[4] == "host"
    for what, g, r in zip(("P", "N", "uv", "indices"), got[:4], ref):
        assert nc.same_bits_or_both_nan(g, r), what
    assert got[0].shape == (du * dv, 3) and got[3].shape == (2 * (du - 1) * (dv - 1), 3)


@pytest.mark.parametrize("name", sorted(nc.CASES))
def test_regular_cases_hold_no_nan(name):
    for du, dv in nc.rates(name):
        assert not any(np.isnan(a).any() for a in nc.restated(name, du, dv)[:3]), (du, dv)


def test_the_degenerate_pole_gives_nan_normals_on_its_row_only():
    P, N, uv, _ = nc.restated("degenerate_pole", 30, 30)
    assert not np.isnan(P).any() and not np.isnan(uv).any()
    assert np.isnan(N[:30]).all() and not np.isnan(N[30:]).any()


def test_the_text_as_it_stands_raises_and_leaves_the_surface(monkeypatch):
    """nurbs.dart:208 and :222-225 unrepaired (nurbs_restatement.REPAIRED = False): beyond the first knot span the iso call of :178 indexes
    at -3 * uFirstCp -- Dart's RangeError --, and the quarter cylinder's x^2 + y^2 runs from 3.06 to 5.86 where r^2 = 4 with a NaN normal at
    vertex 0.  Order 2 on one span is the same either way, byte for byte."""
    import nurbs_restatement as nr
    monkeypatch.setattr(nr, "REPAIRED", False)
    restate = getattr(nc.restated, "__wrapped__")  # past the cache: the cached results are the repaired ones
    with pytest.raises(nr.RangeError):
        restate("multi_span_mixed_order", 4, 4)
    P, N, _, _ = restate("rational_quarter_cylinder", 30, 30)
    r2 = P[:, 0].astype(np.float64) ** 2 + P[:, 1].astype(np.float64) ** 2
    assert r2.min() < 3.1 and r2.max() > 5.8 and np.isnan(N[0]).all()
    assert all(nc.same_bits_or_both_nan(a, b) for a, b in zip(restate("bilinear", 30, 30), nc.restated("bilinear", 30, 30)))


def test_dice_points_land_exactly_on_the_interior_knots():
    """nu = 6, uorder = 4, knots 0 0 0 0 1 2 3 3 3 3 diced 4 times over the whole range: ueval is 0, 1, 2, 3 exactly, so u = 1 and u = 2 are
    interior knots and KnotOffset's `>` keeps each in the span that ENDS there (offsets 3, 3, 4, 5); v = 0, 1, 2, 3 likewise on 0 0 0 1 2 3 3 3.
    The builder's 4 x 4 mesh equals the restatement's (above)."""
    from nurbs_restatement import KnotOffset, Lerp
    ueval = [float(np.float32(Lerp(i / 3, 0.0, 3.0))) for i in range(4)]
    assert ueval == [0.0, 1.0, 2.0, 3.0]
    kw = nc.CASES["multi_span_mixed_order"]
    assert [KnotOffset(kw["uknots"], 4, 6, t) for t in ueval] == [3, 3, 4, 5]
    assert [KnotOffset(kw["vknots"], 3, 5, t) for t in ueval] == [2, 2, 3, 4]
    uv = dice(kw, 4, 4)[2]
    assert uv[:4, 0].tolist() == ueval and uv[::4, 1].tolist() == ueval


def test_the_index_list_is_the_references():
    for du, dv in nc.RATES:
        idx = dice(nc.CASES["bilinear"], du, dv)[3]
        VN = lambda u, v: v * du + u
        want = [[VN(u, v), VN(u + 1, v), VN(u + 1, v + 1), VN(u, v), VN(u + 1, v + 1), VN(u, v + 1)] for v in range(dv - 1) for u in range(du - 1)]
        assert np.array_equal(idx.reshape(-1, 6), np.asarray(want, np.uint32))


def test_the_bilinear_patch_is_its_plane():
    """z = x / 2 + y / 4; order 2 never enters the de Boor loop.  Every point within one f32 ulp of the plane at |z| <= 2 (2^-22 ... the
    point's three roundings), every normal within one f32 ulp (2^-24 .. 2^-23 at these magnitudes) of (-1/2, -1/4, 1) / |.|."""
    for du, dv in nc.RATES:
        P, N, uv, _, _ = dice(nc.CASES["bilinear"], du, dv)
        P64 = P.astype(np.float64)
        assert np.abs(P64[:, 2] - (P64[:, 0] / 2 + P64[:, 1] / 4)).max() <= 2.0 ** -22
        n = np.array([-0.5, -0.25, 1.0]) / np.sqrt(0.25 + 0.0625 + 1.0)
        assert np.abs(N.astype(np.float64) - n).max() <= np.spacing(np.float32(1.0))
        assert uv.min() == 0.0 and uv.max() == 1.0


def test_the_rational_quarter_cylinder_is_a_cylinder():
    """x^2 + y^2 = r^2 and a radial normal.  Tolerance: the weight sqrt(2) / 2 enters as an f32 (relative error 2^-25), a point is three f32
    roundings away from its f64 value and r^2 = 4, so |x^2 + y^2 - 4| <= 8 * 4 * 2^-24 < 2e-6; measured on the restatement's own f32
    output at 30 x 30: 2.4e-7 (x^2 + y^2 from 3.9999998 to 4.0000002).  The normal's components carry the same relative error at |n| = 1."""
    P, N, _, _ = nc.restated("rational_quarter_cylinder", 30, 30)
    P64, N64 = P.astype(np.float64), N.astype(np.float64)
    r2 = P64[:, 0] ** 2 + P64[:, 1] ** 2
    print("x^2 + y^2: %.6g .. %.6g" % (r2.min(), r2.max()))
    assert np.abs(r2 - nc.R ** 2).max() <= 2e-6
    radial = P64[:, :2] / nc.R
    err = np.abs(np.abs(N64[:, :2]) - np.abs(radial)).max()
    print("normal against the radius: %.3g" % err)
    assert err <= 2e-6 and np.abs(N64[:, 2]).max() <= 2e-6


@pytest.mark.parametrize("name", sorted(nc.REFUSALS))
def test_refusals_by_name(name):
    kw, message = nc.REFUSALS[name]
    with pytest.raises(core.DartRayHipError, match="dr_nurbs_dice: .*" + message):
        core.nurbs_dice(builder="host", **kw)


def _patch(kw):
    uk, vk = np.asarray(kw["uknots"], np.float32), np.asarray(kw["vknots"], np.float32)
    cp = np.ascontiguousarray(kw["P"], np.float32)
    patch = _abi.DrNurbsPatch(kw["nu"], kw["uorder"], uk.ctypes.data, kw["u0"], kw["u1"], kw["nv"], kw["vorder"], vk.ctypes.data, kw["v0"],
                              kw["v1"], cp.ctypes.data, 0, 0, 0, 0)
    return patch, (uk, vk, cp)


def test_null_pointers_are_refused_by_name():
    lib = _abi.lib()
    nverts, ntris = C.c_uint64(7), C.c_uint64(7)
    for field, message in ((None, "the patch is null"), ("uknots", "uknots is null"), ("vknots", "vknots is null"), ("cp", "cp is null")):
        patch, keep = _patch(nc.CASES["bezier_bicubic"])
        if field:
            setattr(patch, field, None)
        rc = lib.dr_nurbs_dice(C.byref(patch) if field else None, None, None, None, None, 0, 0, C.byref(nverts), C.byref(ntris))
        assert rc == DR_ERR_INVALID and message in lib.dr_last_error().decode()
        assert (nverts.value, ntris.value) == (7, 7)


def test_size_query_and_capacity_check():
    lib = _abi.lib()
    patch, keep = _patch(nc.CASES["bezier_bicubic"])  # diceu = dicev = 0: the reference's 30
    nverts, ntris = C.c_uint64(0), C.c_uint64(0)
    _abi.check(lib.dr_nurbs_dice(C.byref(patch), None, None, None, None, 0, 0, C.byref(nverts), C.byref(ntris)))
    assert (nverts.value, ntris.value) == (900, 2 * 29 * 29)
    P, N, uv = np.full((900, 3), 7, np.float32), np.full((900, 3), 7, np.float32), np.full((900, 2), 7, np.float32)
    idx = np.full((ntris.value, 3), 7, np.uint32)
    args = (P.ctypes.data, N.ctypes.data, uv.ctypes.data, idx.ctypes.data)
    for vcap, tcap in ((899, ntris.value), (900, ntris.value - 1)):
        assert lib.dr_nurbs_dice(C.byref(patch), *args, vcap, tcap, None, None) == DR_ERR_INVALID
        assert "the output buffers are too small" in lib.dr_last_error().decode()
    assert lib.dr_nurbs_dice(C.byref(patch), P.ctypes.data, None, uv.ctypes.data, idx.ctypes.data, 900, ntris.value, None, None) == DR_ERR_INVALID
    assert "all set or all null" in lib.dr_last_error().decode()
    assert all((a == 7).all() for a in (P, N, uv, idx))  # nothing written
    _abi.check(lib.dr_nurbs_dice(C.byref(patch), *args, 900, ntris.value, None, None))
    got = dice(nc.CASES["bezier_bicubic"])
    assert all(nc.same_bits_or_both_nan(a, b) for a, b in zip((P, N, uv, idx), got[:4]))


def _t(dx, dy, dz):
    m, mi = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
    m[:3, 3], mi[:3, 3] = (dx, dy, dz), (-dx, -dy, -dz)
    return m, mi


def test_bounds_follow_the_reference_formulas():
    """objectBound / worldBound (nurbs.dart:30-70): the union of the control points, the homogeneous branch of x / w, y / w, z / w (f64
    quotients stored f32), worldBound of the transformed points."""
    o2w, w2o = _t(1, -2, 3)
    kw = nc.CASES["bezier_bicubic"]
    a = core.Nurbs(o2w, w2o, False, 4, 4, kw["uknots"], 0, 1, 4, 4, kw["vknots"], 0, 1, kw["P"], False)
    P = np.asarray(kw["P"], np.float32)
    assert not a.canIntersect()
    assert np.array_equal(a.objectBound()[0], P.min(0)) and np.array_equal(a.objectBound()[1], P.max(0))
    Pw_ = core.transform_points(o2w, P)
    assert np.array_equal(a.worldBound()[0], Pw_.min(0)) and np.array_equal(a.worldBound()[1], Pw_.max(0))
    kw = nc.CASES["rational_quarter_cylinder"]
    h = core.Nurbs(o2w, w2o, False, 3, 3, kw["uknots"], 0, 1, 2, 2, kw["vknots"], 0, 1, kw["Pw"], True)
    Pw = np.asarray(kw["Pw"], np.float32).astype(np.float64)
    pts = np.array([[np.float32(p[0] / p[3]), np.float32(p[1] / p[3]), np.float32(p[2] / p[3])] for p in Pw], np.float32)
    assert np.array_equal(h.objectBound()[0], pts.min(0)) and np.array_equal(h.objectBound()[1], pts.max(0))
    assert np.array_equal(h.objectBound()[1], np.float32([nc.R, nc.R, nc.H]))
    ptsw = core.transform_points(o2w, pts)
    assert np.array_equal(h.worldBound()[0], ptsw.min(0)) and np.array_equal(h.worldBound()[1], ptsw.max(0))


def _numbers(a, fmt="%.17g"):  # enough digits to name the f32 exactly
    return " ".join(fmt % c for c in np.asarray(a, np.float64).reshape(-1))


def nurbs_directive(kw):
    cp = '"point P" [%s]' % _numbers(kw["P"]) if "P" in kw else '"float Pw" [%s]' % _numbers(np.asarray(kw["Pw"], np.float32))
    return ('Shape "nurbs" "integer nu" [%d] "integer uorder" [%d] "float uknots" [%s] "float u0" [%s] "float u1" [%s] '
            '"integer nv" [%d] "integer vorder" [%d] "float vknots" [%s] "float v0" [%s] "float v1" [%s] %s'
            % (kw["nu"], kw["uorder"], _numbers(kw["uknots"]), _numbers(kw["u0"]), _numbers(kw["u1"]), kw["nv"], kw["vorder"],
               _numbers(kw["vknots"]), _numbers(kw["v0"]), _numbers(kw["v1"]), cp))


@pytest.mark.parametrize("name,reverse", [("sub_range", False), ("rational_quarter_cylinder", True)])
def test_loader_yields_the_mesh_of_core_nurbs(name, reverse):
    kw = nc.CASES[name]
    warnings = []
    api = pbrt.loads("WorldBegin\nTranslate 1 2 3\nRotate 30 0 1 0\n%s%s\nWorldEnd\n" % ("ReverseOrientation\n" if reverse else "", nurbs_directive(kw)),
                     warn=warnings.append)
    assert warnings == []
    mesh = api.primitives[0].shape
    ctm = pbrt.Transform.Translate(1, 2, 3) * pbrt.Transform.Rotate(30, 0, 1, 0)
    homogeneous = "Pw" in kw
    want = core.Nurbs(ctm.m, ctm.mInv, reverse, kw["nu"], kw["uorder"], kw["uknots"], kw["u0"], kw["u1"], kw["nv"], kw["vorder"], kw["vknots"],
                      kw["v0"], kw["v1"], kw["Pw"] if homogeneous else kw["P"], homogeneous).refine(builder="host")
    assert isinstance(mesh, core.TriangleMesh) and mesh.reverseOrientation is reverse
    assert mesh.n is not None and mesh.uvs is not None and len(mesh.P) == 900
    for a, b in ((mesh.P, want.P), (mesh.n, want.n), (mesh.uvs, want.uvs), (mesh.vertexIndex, want.vertexIndex),
                 (mesh.objectToWorld, want.objectToWorld), (mesh.worldToObject, want.worldToObject)):
        assert nc.same_bits_or_both_nan(a, b)
    assert np.array_equal(mesh.objectToWorld, ctm.m) and np.array_equal(mesh.worldToObject, ctm.mInv)


def test_loader_defaults_and_dropped_shapes():
    head = 'Shape "nurbs" "integer nu" [2] "integer uorder" [2] "float uknots" [0 0 1 1] "integer nv" [2] "integer vorder" [2] "float vknots" [0 0 1 1] '
    api = pbrt.loads("WorldBegin\n" + head + '"point P" [0 0 0 2 0 1 0 4 1 2 4 2]\nWorldEnd\n')  # u0 .. v1 default to the knot range
    assert nc.same_bits_or_both_nan(api.primitives[0].shape.P, dice(nc.CASES["bilinear"])[0])
    for cp in ('', '"float Pw" [0 0 0 1 2 0 1 1 0 4 1]', '"point P" [0 0 0 2 0 1 0 4 1]'):  # none; no multiple of four; not nu * nv
        warnings = []
        api = pbrt.loads("WorldBegin\n" + head + cp + "\nWorldEnd\n", warn=warnings.append)
        assert api.primitives == [] and any("NURBS shape" in w for w in warnings)
    with pytest.raises(pbrt.UnsupportedFeature, match=r"<string>:3: Shape \"nurbs\": 3 uknots, expected nu \+ uorder = 4"):
        pbrt.loads("WorldBegin\n\n" + head.replace('"float uknots" [0 0 1 1]', '"float uknots" [0 0 1]') + '"point P" [0 0 0 2 0 1 0 4 1 2 4 2]\nWorldEnd\n')
    with pytest.raises(pbrt.UnsupportedFeature, match="Shape \"cylinder\": only .*'nurbs'"):
        pbrt.loads('WorldBegin\nShape "cylinder"\nWorldEnd\n')
    warnings = []
    pbrt.loads("WorldBegin\n" + head.replace('[0 0 1 1] "integer nv"', '[0 0 0.1 0.1] "integer nv"') + '"point P" [0 0 0 2 0 1 0 4 1 2 4 2]\nWorldEnd\n',
               warn=warnings.append)
    assert any("rounded to f32" in w for w in warnings)


def test_header_binding_and_dart_name_the_entry_points():
    header = open(os.path.join(ROOT, "include", "dartray_hip.h")).read()
    dart = open(os.path.join(ROOT, "integration", "hip_sampler_renderer.dart")).read()
    for name in ("dr_nurbs_dice", "dr_nurbs_dice_device"):
        assert "int %s(const DrNurbsPatch* patch" % name in header and name in _abi.EXPORTS and "'%s'" % name in dart
    assert C.sizeof(_abi.DrNurbsPatch) == 72 and "const int SIZEOF_DrNurbsPatch = 72;" in dart
    for field, _ in _abi.DrNurbsPatch._fields_[:-1]:
        assert "const int OFF_DrNurbsPatch_%s = %d;" % (field, getattr(_abi.DrNurbsPatch, field).offset) in dart
    assert "#define DR_NURBS_MAX_ORDER %d" % _abi.DR_NURBS_MAX_ORDER in header


def test_host_builder_runs_clean_under_the_sanitizers(tmp_path):
    """tests/nurbs_host_check.cpp + dr_nurbs_host.cpp, built with -fsanitize=address,undefined and run as a child process; the sanitizer
    runtimes are linked into the program, which then depends on nothing else the process loads."""
    exe = str(tmp_path / "nurbs_host_check")
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "nurbs_host_check.cpp"),
                           os.path.join(ROOT, "dartray_amd", "csrc", "dr_nurbs_host.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "nurbs_host_check: OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
