"""The figures of MEASUREMENTS.md, "The glossy PRT integrator": the once-per-scene cost of the BSDF matrix at 1024 directions, then three renders
each of GlossyPRTIntegrator(lmax 4, 256 rays) and DiffusePRTIntegrator(4, 256) on the yard scene of tests/test_gpu_glossy_prt.py at 256 x 256,
1 spp.  Run from the repository root on a GPU:

    python tools/measure_glossy_prt.py
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o gprt -- python tools/measure_glossy_prt.py   # per-kernel durations
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dartray_amd import _abi, core  # noqa: E402

KD, KS, ROUGH = (0.6, 0.45, 0.3), (0.2, 0.25, 0.35), 0.1
FLOOR = ((-4.0, 0.0, -4.0), (-4.0, 0.0, 6.0), (4.0, 0.0, 6.0), (4.0, 0.0, -4.0))
BLOCKER = ((0.0, 1.5, -1.0), (3.0, 1.5, -1.0), (3.0, 1.5, 3.0), (0.0, 1.5, 3.0))
UP = ((-3.0, 1.5, -1.0), (-3.0, 1.5, 3.0), (0.0, 1.5, 3.0), (0.0, 1.5, -1.0))
LEANING = ((-2.5, 0.2, -2.5), (-2.5, 1.2, -1.5), (-0.3, 1.2, -1.5), (-0.3, 0.2, -2.5))
LEANING_N = np.array([(0.3, 0.7, -0.6), (-0.2, 0.9, -0.3), (-0.3, 0.8, -0.5), (0.4, 0.6, -0.7)], np.float32)


def quad(p, kd=(0.5, 0.5, 0.5), light=None, **kw):
    mesh = core.TriangleMesh(np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.array(p, np.float32), **kw)
    return core.GeometricPrimitive(mesh, core.MatteMaterial(kd), core.DiffuseAreaLight(light[0], light[1], mesh) if light else None)


def main(res=256, lmax=4, rays=256):
    _abi.init(0)
    accel = core.BVHAccel([quad(FLOOR), quad(UP, light=((6.0, 5.0, 4.0), 1)), quad(LEANING, kd=(0.6, 0.5, 0.4), n=LEANING_N), quad(BLOCKER)])
    scene = core.Scene(accel, accel.lights() + [core.InfiniteAreaLight(None, (0.8, 0.9, 1.0), 1, None)])
    cam = core.PerspectiveCamera.lookAt((0.5, 5.0, -7.0), (0.0, 0.5, 1.0), (0.0, 1.0, 0.0), 80.0, core.ImageFilm(res, res, core.BoxFilter(0.5, 0.5)))
    glossy = core.GlossyPRTIntegrator(KD, KS, ROUGH, lmax, rays)
    for what, integ in (("with the incident light, first call", glossy), ("another Ks, incident light cached", core.GlossyPRTIntegrator(KD, 0.1, ROUGH, lmax, rays))):
        t0 = time.perf_counter()
        integ.bsdf_matrix(scene, 1024)
        print("B at 1024, lmax %d (%s): %.1f ms wall" % (lmax, what, (time.perf_counter() - t0) * 1e3))
    for name, integ in (("glossy", glossy), ("diffuse", core.DiffusePRTIntegrator(lmax, rays))):
        r = core.SamplerRenderer(core.LowDiscrepancySampler(cam, 1, 5489), cam, integ, core.EmissionIntegrator())
        for k in range(3):
            r.render(scene)
            st = r.last_stats
            print("%s render %d: total %.1f ms, any-hit %.1f ms, shading %.1f ms, %d any-hit rays in %d launches, %d hits"
                  % (name, k, st["total_ms"], st["any_ms"], st["shade_ms"], st["any_rays"], st["any_launches"], st["shade_vertices"]))


if __name__ == "__main__":
    main()
