"""Host-side mirror of the reference's plugin interface for the hot path.

The reference is Dart; no Dart SDK exists in this image, so the host code above
the C ABI is written in Python with the reference's class names, constructor
arguments and error behaviour (a failing native call raises, like LogSevere,
lib/core/log.dart:42-47).  Each class cites the Dart class it mirrors; the
compute itself happens in libdartray_hip.so.

    prims   = [GeometricPrimitive(TriangleMesh(...), MatteMaterial(Kd), DiffuseAreaLight(L) or None), ...]
    accel   = BVHAccel(prims)                               # lib/accelerators/bvh_accel.dart
    scene   = Scene(accel, lights)                          # lib/core/scene.dart
    film    = ImageFilm(64, 64, BoxFilter(0.5, 0.5))        # lib/film/image_film.dart
    camera  = PerspectiveCamera.lookAt(pos, look, up, fov, film)
    sampler = LowDiscrepancySampler(camera, 4)
    out     = SamplerRenderer(sampler, camera, PathIntegrator(5), EmissionIntegrator()).render(scene)

One module per directory of the reference's lib/ (transform.py: the matrix part of lib/core/ that shapes, lights and cameras share).  A new
material, light, shape or sampler class goes into its module; its to_abi is the only marshalling it needs.
"""
import ctypes as C  # noqa: F401  (core.py exposed the modules it imported; the names stay)
import collections  # noqa: F401
import math  # noqa: F401
import os  # noqa: F401

import numpy as np  # noqa: F401

from .. import _abi  # noqa: F401
from .._abi import DartRayHipError  # noqa: F401  (re-export)
from .transform import _bbox_transform, _inv, _m4, _mul, _normalize, look_at, transform_points  # noqa: F401
from .shapes import Disk, LoopSubdivision, Sphere, TriangleMesh, _Quadric, loop_subdivide  # noqa: F401
from .shapes import Nurbs, nurbs_dice  # noqa: F401  (core.Nurbs / core.nurbs_dice; not in __all__: the package's star-import list is recorded)
from .materials import GlassMaterial, MatteMaterial, MirrorMaterial, PlasticMaterial  # noqa: F401
from .lights import DiffuseAreaLight, DistantLight, InfiniteAreaLight, PointLight, SpotLight, delta_light_kind  # noqa: F401
from .accel import (HIT_DTYPE, NODE_DTYPE, BVHAccel, GeometricPrimitive, Ray, Scene, _DeviceScene, build_bvh_arrays,  # noqa: F401
                    describe_scene)
from .film import FILTER_TABLE_SIZE, BoxFilter, Filter, GaussianFilter, ImageFilm, LanczosSincFilter, MitchellFilter, TriangleFilter  # noqa: F401
from .cameras import EnvironmentCamera, OrthographicCamera, PerspectiveCamera, _default_screen_window, _raster_to_screen  # noqa: F401
from .samplers import (ONE_MINUS_EPSILON, AdaptiveSampler, DartRandom, GetSubWindow, HaltonSampler, HostBufferSampler, Lerp,  # noqa: F401
                       LinearPixelSampler, LowDiscrepancySampler, RadicalInverse, RandomPixelSampler, RandomSampler, RoundUpPow2, StratifiedSampler,
                       TilePixelSampler, _latin_hypercube_slots, _pack_tails)
from .renderer import (AmbientOcclusionIntegrator, DiffusePRTIntegrator, DirectLightingIntegrator, EmissionIntegrator, FeatureIntegrator, GlossyPRTIntegrator, MaterialIntegrator, OutputImage, PathIntegrator,  # noqa: F401
                       ProbeGrid, SamplerRenderer, UseProbesIntegrator, WhittedIntegrator)
from .plugins import Plugin, RegisterStandardPlugins  # noqa: F401

# what `from dartray_amd import *` binds: core.py's public names, the five modules it had imported among them (a recorded list: classes added
# since -- RandomSampler, WhittedIntegrator, AmbientOcclusionIntegrator, FeatureIntegrator, DiffusePRTIntegrator, GlossyPRTIntegrator, UseProbesIntegrator, ProbeGrid, MaterialIntegrator -- are reached as core.<name>)
__all__ = [
    "C", "collections", "math", "np", "os", "DartRayHipError",
    "look_at", "transform_points",
    "Disk", "LoopSubdivision", "Sphere", "TriangleMesh", "loop_subdivide",
    "GlassMaterial", "MatteMaterial", "MirrorMaterial", "PlasticMaterial",
    "DiffuseAreaLight", "DistantLight", "InfiniteAreaLight", "PointLight", "SpotLight", "delta_light_kind",
    "HIT_DTYPE", "NODE_DTYPE", "BVHAccel", "GeometricPrimitive", "Ray", "Scene", "build_bvh_arrays",
    "FILTER_TABLE_SIZE", "BoxFilter", "Filter", "GaussianFilter", "ImageFilm", "LanczosSincFilter", "MitchellFilter", "TriangleFilter",
    "EnvironmentCamera", "OrthographicCamera", "PerspectiveCamera",
    "ONE_MINUS_EPSILON", "AdaptiveSampler", "DartRandom", "GetSubWindow", "HaltonSampler", "HostBufferSampler", "Lerp",
    "LinearPixelSampler", "LowDiscrepancySampler", "RadicalInverse", "RandomPixelSampler", "RoundUpPow2", "StratifiedSampler",
    "TilePixelSampler",
    "DirectLightingIntegrator", "EmissionIntegrator", "OutputImage", "PathIntegrator", "SamplerRenderer",
    "Plugin", "RegisterStandardPlugins",
]
