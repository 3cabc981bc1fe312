"""The first-hit material integrator restated in plain Python -- the test side's own reading of the reference text the section
cites, on top of the scene, shapes, camera and film of tests/feature_restatement.py and the lights of tests/golden/dart_restatement.py (imported,
not copied).  What is stated here is the two values and nothing else:

    albedo    the colour the hit's material hands its first lobe: Kd.evaluate(dgs).clamp() of matte (matte_material.dart:54) and plastic
              (plastic_material.dart:52), Kr.evaluate(dgs).clamp() of mirror (mirror_material.dart:44) and glass (glass_material.dart:52); a miss: 0
    emission  what Li adds for the camera ray itself (path_integrator.dart:46-48, direct_lighting_integrator.dart:40, whitted_integrator.dart:40):
              isect.Le(-ray.d) (intersection.dart:60-63) = area.L(dg.p, dg.nn, wo) (diffuse_area_light.dart:44-46); a miss: the sum of every
              light's Le(ray) (sampler_renderer.dart:86-92; infinite_area_light.dart:84-90; light.dart:70-72)

Shares no code with the library: the scene arrives as the flat arrays dr_scene_create receives."""
import math

import numpy as np

import feature_restatement as fe
from feature_restatement import dr, RGB

ALBEDO, EMISSION = 0, 1                                            # DR_MATERIAL_CHANNEL_* (include/dartray_hip.h)
CHANNELS = {"albedo": ALBEDO, "emission": EMISSION}


class AreaLight:
    """The two methods of a DiffuseAreaLight an emission image reads (its ShapeSet is for sampling, which nothing here does)."""

    def __init__(self, Lemit):
        self.Lemit = RGB(*Lemit)

    def L(self, n, w):                                             # diffuse_area_light.dart:44-46
        return self.Lemit if dr.Dot(n, w) > 0.0 else RGB(0.0)

    def Le(self, ray):                                             # light.dart:70-72: an area light adds nothing to an escaped ray
        return RGB(0.0)


class MaterialScene:
    """bvh: fe.FlatScene's; every prim carries .colour (an RGB: the material's Kd or Kr) and .light (an AreaLight or None);
    lights: every light of the scene, in its order (area lights among them: their Le(ray) is 0)."""

    def __init__(self, bvh, lights):
        self.bvh, self.lights = bvh, lights


def build_scene(flat, materials, tri_light, lights):
    """flat: fe.build_scene(...) of the aggregate.  materials[m] = ("matte" | "plastic" | "mirror" | "glass", Kd, Kr), the material table;
    tri_light[i]: the position of primitive i's area light in `lights`, or -1; lights[k] = ("area", Lemit) or
    ("infinite", lightToWorld, worldToLight, L, texels, width, height)."""
    made = []
    for l in lights:
        if l[0] == "area":
            made.append(AreaLight(tuple(float(v) for v in l[1])))
        else:
            made.append(dr.InfiniteAreaLight(l[1], l[2], tuple(float(v) for v in l[3]), [tuple(float(v) for v in t) for t in l[4]], l[5], l[6]))
    for i, p in enumerate(flat.bvh.prims):
        kind, kd, kr = materials[p.ids[1]]
        c = kr if kind in ("mirror", "glass") else kd
        p.colour = RGB(float(c[0]), float(c[1]), float(c[2]))
        p.light = made[int(tri_light[i])] if int(tri_light[i]) >= 0 else None
    return MaterialScene(flat.bvh, made)


def Li(scene, channel, ray, isect):
    """DESIGN.md 2.27, at a hit."""
    if channel == ALBEDO:
        return isect.prim.colour.clamp()                           # Spectrum.clamp(): below 0 -> 0 (rgb_color.dart:189-192)
    assert channel == EMISSION
    return dr.isect_Le(isect, -ray.d)                              # intersection.dart:60-63 -> diffuse_area_light.dart:44-46


def Li_miss(scene, channel, ray):
    if channel == ALBEDO:
        return RGB(0.0)
    L = RGB(0.0)
    for light in scene.lights:                                     # sampler_renderer.dart:89-91
        L = L + light.Le(ray)
    return L


def sample_Li(scene, channel, camera, px, py, sv):
    """One camera sample, as fe.sample_Li: generateRay, intersect, Li, T * Li + Lv with T = 1 and Lv = 0, * rayWeight, the guards."""
    imageX = px + float(sv[0])
    imageY = py + float(sv[1])
    ray = camera.generateRay(imageX, imageY, float(sv[2]), float(sv[3]))
    isect = scene.bvh.intersect(ray)
    L = Li(scene, channel, ray, isect) if isect is not None else Li_miss(scene, channel, ray)
    Ls = (RGB(1.0) * L + RGB(0.0)) * 1.0
    if Ls.hasNaNs():
        Ls = RGB(0.0)
    elif Ls.luminance() < -1e-5:
        Ls = RGB(0.0)
    elif math.isinf(Ls.luminance()):
        Ls = RGB(0.0)
    return Ls, imageX, imageY, isect is not None


def render(scene, channel, camera, xres, yres, xWidth, yWidth, filterTable, spp, pixels, vectors):
    """fe.render over this file's sample_Li -> (Ls [n][3] f32, hit [n] bool, film [H][W][4] f32, rgb [H][W][3] f32)."""
    film = dr.ImageFilm(xres, yres, xWidth, yWidth, filterTable)
    Ls, hits = [], []
    for k, (px, py) in enumerate(np.asarray(pixels).reshape(-1, 2)):
        pending = []
        for i in range(spp):
            L, ix, iy, hit = sample_Li(scene, channel, camera, int(px), int(py), vectors[k * spp + i])
            pending.append((ix, iy, L))
            Ls.append(L.tuple())
            hits.append(hit)
        for a in pending:
            film.addSample(*a)
    lx = np.array(film.Lxyz, np.float32).reshape(yres, xres, 3)
    out = np.concatenate([lx, np.array(film.weightSum, np.float32).reshape(yres, xres, 1)], axis=2)
    return np.array(Ls, np.float32), np.array(hits, bool), out, np.array(film.writeImage(), np.float32).reshape(yres, xres, 3)
